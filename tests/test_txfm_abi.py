"""CPU: the C-ABI of the TX chain's FM mode (include/selenite_tx_fm.h, which include/selenite_tx.h includes: selenite_tx_set_fm,
selenite_tx_get_fm_state, selenite_tx_set_fm_state, selenite_tx_tone_step) is exported and bound, the ctypes structs lay out as the C
compiler does, and the entry points refuse a NULL instance without touching a GPU.  (That every bad field of the config is refused with the
old setting left in place needs an instance: tests/test_gpu_txfm.py.)"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import rxcommon as rc
import selenite_rx as sr

NAMES = {"selenite_tx_set_fm": 2, "selenite_tx_get_fm_state": 2, "selenite_tx_set_fm_state": 2, "selenite_tx_tone_step": 2}
CONFIG_FIELDS = ("struct_size", "deviation", "amplitude", "tone_enable", "tone_level", "tone_step_all", "tone_step", "reserved")
VIEW_FIELDS = ("tone_phase",)


def test_symbols_exported_and_bound():
    L = sr.lib()
    text = open(os.path.join(rc.ROOT, "include", "selenite_tx_fm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(selenite_tx_[a-z0-9_]+)\s*\(", code))) == sorted(NAMES) == sorted(sr.TXFM_ABI_SYMBOLS)
    for n, nargs in NAMES.items():
        assert hasattr(L, n), n
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == nargs
    for decl in ("int selenite_tx_set_fm(selenite_tx_instance *S, const selenite_tx_fm_config *cfg);",
                 "int selenite_tx_get_fm_state(selenite_tx_instance *S, const selenite_tx_fm_state_view *view);",
                 "int selenite_tx_set_fm_state(selenite_tx_instance *S, const selenite_tx_fm_state_view *view);",
                 "uint32_t selenite_tx_tone_step(double hz, double fs_out);"):
        assert decl in text, decl
    assert '#include "selenite_tx_fm.h"' in open(os.path.join(rc.ROOT, "include", "selenite_tx.h")).read()      # one header to include
    for m in ("set_fm", "fm_state", "set_fm_state"):
        assert callable(getattr(sr.Tx, m))
    assert callable(sr.tone_step)


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_tx.h"
#define O(f) offsetof(selenite_tx_fm_config, f)
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_tx_fm_config), O(struct_size), O(deviation), O(amplitude), O(tone_enable),
           O(tone_level), O(tone_step_all), O(tone_step), O(reserved));
    printf("%zu %zu\n", sizeof(selenite_tx_fm_state_view), offsetof(selenite_tx_fm_state_view, tone_phase));
    printf("%zu\n", sizeof(selenite_tx_config));
    return 0;
}
"""


def test_ctypes_layout_equals_offsetof():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(C_SNIPPET)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(rc.ROOT, "include"), "-o", exe, src], check=True)
        lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    assert [int(v) for v in lines[0].split()] == [C.sizeof(sr.TxFmConfig)] + [getattr(sr.TxFmConfig, f).offset for f in CONFIG_FIELDS]
    assert [int(v) for v in lines[1].split()] == [C.sizeof(sr.TxFmStateView)] + [getattr(sr.TxFmStateView, f).offset for f in VIEW_FIELDS]
    assert C.sizeof(sr.TxFmConfig) == 40 and sr.TxFmConfig.tone_step.offset == 24 and C.sizeof(sr.TxFmStateView) == 8
    assert [f for f, _ in sr.TxFmConfig._fields_] == list(CONFIG_FIELDS) and [f for f, _ in sr.TxFmStateView._fields_] == list(VIEW_FIELDS)
    assert int(lines[2]) == C.sizeof(sr.TxConfig) == 104            # selenite_tx_config does not change


def test_null_instance_is_an_argument_error():
    L = sr.lib()
    g = sr.TxFmConfig()
    g.struct_size, g.deviation, g.amplitude = C.sizeof(sr.TxFmConfig), 0.25, 1.0
    assert L.selenite_tx_set_fm(None, C.byref(g)) == sr.ARGUMENT_ERROR
    assert L.selenite_tx_set_fm(None, None) == sr.ARGUMENT_ERROR
    tp = np.full(4, 7, np.uint32)
    v = sr.TxFmStateView()
    v.tone_phase = tp.ctypes.data_as(sr.u32p)
    assert L.selenite_tx_get_fm_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_tx_set_fm_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_tx_get_fm_state(None, None) == sr.ARGUMENT_ERROR
    assert (tp == 7).all()
