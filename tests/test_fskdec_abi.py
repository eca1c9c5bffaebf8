"""CPU: the FSK teleprinter decoder's C-ABI (include/selenite_rx.h: selenite_rx_set_fskdec, selenite_rx_get_fskdec_state,
selenite_rx_set_fskdec_state, selenite_rx_get_fskdec, selenite_rx_fskdec_text_device, selenite_rx_fskdec_count_device,
selenite_rx_fskdec_lvl_device, selenite_rx_design_fsk, selenite_rx_design_ita2) is exported and bound, the ctypes structs lay out as the C
compiler does, the older structs keep their sizes, the entry points refuse a NULL instance and bad arguments without touching a GPU, and the
design helpers give what the restatement uses.  (That every range check of the config refuses with a working stage left in place needs an
instance: tests/test_gpu_fskdec.py.)"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fskdec_oracle as fo
import rxcommon as rc
import selenite_rx as sr

NAMES = {"selenite_rx_set_fskdec": 2, "selenite_rx_get_fskdec_state": 2, "selenite_rx_set_fskdec_state": 2, "selenite_rx_get_fskdec": 5,
         "selenite_rx_fskdec_text_device": 1, "selenite_rx_fskdec_count_device": 1, "selenite_rx_fskdec_lvl_device": 1,
         "selenite_rx_design_fsk": 5, "selenite_rx_design_ita2": 1}
CONFIG_FIELDS = ("struct_size", "tick", "bit_q8", "reverse", "usos", "ring", "mark", "space", "alpha", "hyst", "frac", "min_power", "table")
VIEW_FIELDS = ("filt", "em", "es", "ew", "lvl", "k", "t_q8", "shift", "figs", "ferr", "bit", "count", "text")


def test_symbols_exported_and_bound():
    L = sr.lib()
    for n, nargs in NAMES.items():
        assert hasattr(L, n), n
        assert n in sr.ABI_SYMBOLS
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == nargs
    text = open(os.path.join(rc.ROOT, "include", "selenite_rx.h")).read()
    for decl in ("int selenite_rx_set_fskdec(selenite_rx_instance *S, const selenite_rx_fskdec_config *f);",
                 "int selenite_rx_get_fskdec_state(selenite_rx_instance *S, const selenite_rx_fskdec_state_view *dst);",
                 "int selenite_rx_set_fskdec_state(selenite_rx_instance *S, const selenite_rx_fskdec_state_view *src);",
                 "int selenite_rx_get_fskdec(selenite_rx_instance *S, uint8_t *text, uint64_t *count, uint32_t *ferr, uint32_t *lvl);",
                 "const uint8_t *selenite_rx_fskdec_text_device(const selenite_rx_instance *S);",
                 "const uint64_t *selenite_rx_fskdec_count_device(const selenite_rx_instance *S);",
                 "const uint32_t *selenite_rx_fskdec_lvl_device(const selenite_rx_instance *S);",
                 "int selenite_rx_design_fsk(double f_mark, double f_space, double bandwidth, float mark[5], float space[5]);",
                 "int selenite_rx_design_ita2(uint8_t table[64]);"):
        assert decl in text, decl
    assert "#define SELENITE_RX_ABI_VERSION 2" in text and L.selenite_rx_abi_version() == 2 and sr.ABI_VERSION == 2      # (a new stage, not a new version)
    for m in ("set_fskdec", "fskdec_state", "set_fskdec_state", "fskdec", "fsk_text", "fsk_lvl", "fskdec_text_device", "fskdec_count_device",
              "fskdec_lvl_device"):
        assert callable(getattr(sr.Rx, m))
    assert callable(sr.fsk_bandpass) and callable(sr.ita2_table)
    for n in ("selenite_rx_fskdec_text_device", "selenite_rx_fskdec_count_device", "selenite_rx_fskdec_lvl_device"):
        assert sr.SIGNATURES[n][0] is C.c_void_p


def test_the_law_stands_word_for_word_in_the_header_the_kernel_file_and_the_design():
    """every line of the law between `two arm_biquad_cascade_df1_f32 instances` and `emit(b):`, less the comment leaders"""
    def law(path, lead):
        lines = [ln.strip() for ln in open(os.path.join(rc.ROOT, path)).read().split("\n")]
        lines = [ln[len(lead):].strip() if ln.startswith(lead) else ln for ln in lines]
        a = next(i for i, ln in enumerate(lines) if ln.startswith("two arm_biquad_cascade_df1_f32 instances of ONE section each"))
        b = next(i for i, ln in enumerate(lines) if ln.startswith("emit(b):"))
        return [" ".join(ln.split()) for ln in lines[a:b + 1]]
    h = law("include/selenite_rx.h", "*")
    assert len(h) == 27
    assert h == law("selenite-lite_amd/csrc/rx_fskdec.hip", "//")
    assert h == law("DESIGN.md", "")


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_rx.h"
#define O(f) offsetof(selenite_rx_fskdec_config, f)
#define V(f) offsetof(selenite_rx_fskdec_state_view, f)
#define Z(t) sizeof(selenite_rx_##t)
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_fskdec_config), O(struct_size), O(tick), O(bit_q8),
           O(reverse), O(usos), O(ring), O(mark), O(space), O(alpha), O(hyst), O(frac), O(min_power), O(table));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_fskdec_state_view), V(filt), V(em), V(es), V(ew), V(lvl),
           V(k), V(t_q8), V(shift), V(figs), V(ferr), V(bit), V(count), V(text));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", Z(config), Z(state_view), Z(nr_config), Z(nr_state_view), Z(nb_config),
           Z(iqc_config), Z(meter_config), Z(meter_state_view), Z(afilt_config), Z(afilt_state_view), Z(tones_config), Z(tones_state_view),
           Z(cwdec_config), Z(cwdec_state_view), Z(nb_state_view), Z(iqc_state_view));
    return 0;
}
"""
# sizeof of the structs that were there before the stage, as the parent's header gave them
OLDER = dict(Config=None, StateView=None, NrConfig=None, NrStateView=None, NbConfig=None, IqcConfig=None, MeterConfig=36, MeterStateView=40,
             AfiltConfig=24, AfiltStateView=16, TonesConfig=40, TonesStateView=80, CwdecConfig=72, CwdecStateView=88, NbStateView=24,
             IqcStateView=40)


def test_ctypes_layout_equals_offsetof_and_the_older_structs_keep_their_sizes():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(C_SNIPPET)
        subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(rc.ROOT, "include"), "-o", exe, src], check=True)
        lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    assert [int(v) for v in lines[0].split()] == [C.sizeof(sr.FskdecConfig)] + [getattr(sr.FskdecConfig, f).offset for f in CONFIG_FIELDS]
    assert [int(v) for v in lines[1].split()] == [C.sizeof(sr.FskdecStateView)] + [getattr(sr.FskdecStateView, f).offset for f in VIEW_FIELDS]
    assert C.sizeof(sr.FskdecConfig) == 88 and C.sizeof(sr.FskdecStateView) == 104
    assert [f for f, _ in sr.FskdecConfig._fields_] == list(CONFIG_FIELDS) and [f for f, _ in sr.FskdecStateView._fields_] == list(VIEW_FIELDS)
    assert sr.Rx.FSKDEC_TYPES.keys() == set(VIEW_FIELDS) and list(sr.Rx.FSKDEC_TYPES) == list(VIEW_FIELDS) == list(fo.ROWS)
    assert all(sr.Rx.FSKDEC_TYPES[k] is fo.ROWS[k] for k in VIEW_FIELDS)
    # the header's older structs: what the C compiler says, what ctypes says, and where a figure is on record, that figure
    for size, (name, known) in zip((int(v) for v in lines[2].split()), OLDER.items()):
        assert size == C.sizeof(getattr(sr, name)), name
        assert known is None or size == known, name


def config(**over):
    g = sr.FskdecConfig()
    g.struct_size = C.sizeof(sr.FskdecConfig)
    for k, v in dict(sr.FSKDEC_DEFAULTS, **over).items():
        setattr(g, k, v)
    m, s = sr.fsk_bandpass(2125.0 / 12000.0, 2295.0 / 12000.0, 90.0 / 12000.0)
    g.mark[:], g.space[:] = m.tolist(), s.tolist()
    return g


def test_null_instance_is_an_argument_error():
    L = sr.lib()
    assert L.selenite_rx_set_fskdec(None, C.byref(config())) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_fskdec(None, None) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_error_string(None)
    text, count, ferr, lvl = np.full(64, 7, np.uint8), np.full(4, 9, np.uint64), np.full(4, 5, np.uint32), np.full(4, 3, np.uint32)
    v = sr.FskdecStateView()
    v.text, v.count, v.ferr, v.lvl = text.ctypes.data_as(sr.u8p), count.ctypes.data_as(sr.u64p), ferr.ctypes.data_as(sr.u32p), lvl.ctypes.data_as(sr.u32p)
    assert L.selenite_rx_get_fskdec_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_fskdec_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_get_fskdec_state(None, None) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_get_fskdec(None, v.text, v.count, v.ferr, v.lvl) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_fskdec_text_device(None) is None and L.selenite_rx_fskdec_count_device(None) is None
    assert L.selenite_rx_fskdec_lvl_device(None) is None
    assert (text == 7).all() and (count == 9).all() and (ferr == 5).all() and (lvl == 3).all()


def test_the_defaults_are_the_documented_ones():
    assert sr.FSKDEC_DEFAULTS == dict(tick=16, bit_q8=4224, reverse=0, usos=1, ring=256, alpha=0.25, hyst=0.1, frac=0.35, min_power=1e-6)
    assert fo.DEFAULTS == sr.FSKDEC_DEFAULTS and fo.bit_q8(12000.0, 45.45, 16) == 4224
    for k in sr.FSKDEC_DEFAULTS:
        assert k in sr.Rx.set_fskdec.__doc__, k


def test_design_fsk_against_the_restatement_and_its_refusals():
    L = sr.lib()
    for fm, fs, bw in ((2125.0 / 12000.0, 2295.0 / 12000.0, 90.0 / 12000.0), (0.15, 0.20, 0.02), (1275.0 / 8000.0, 1445.0 / 8000.0, 140.0 / 8000.0)):
        m, s = sr.fsk_bandpass(fm, fs, bw)
        om, osp = fo.design(fm, fs, bw)
        assert m.tobytes() == om.tobytes() and s.tobytes() == osp.tobytes()
        # the constant-peak-gain band-pass: b1 = 0, b2 = -b0, unit gain at the centre: |H(w0)| = 1 within the rounding of five floats
        for c, f0 in ((m, fm), (s, fs)):
            assert c[1] == 0 and c[2] == -c[0] and c[0] > 0
            z = np.exp(-2j * np.pi * f0)
            h = (c[0] + c[1] * z + c[2] * z * z) / (1.0 - c[3] * z - c[4] * z * z)
            assert abs(abs(h) - 1.0) < 1e-4
    a, b = np.zeros(5, np.float32), np.zeros(5, np.float32)
    fp = lambda v: v.ctypes.data_as(sr.f32p)      # noqa: E731
    assert L.selenite_rx_design_fsk(0.1, 0.2, 0.01, None, fp(b)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_design_fsk(0.1, 0.2, 0.01, fp(a), None) == sr.ARGUMENT_ERROR
    for bad in ((0.0, 0.2, 0.01), (0.1, 0.5, 0.01), (0.1, 0.2, 0.0), (float("nan"), 0.2, 0.01), (0.1, 0.2, float("inf")), (-0.1, 0.2, 0.01)):
        assert L.selenite_rx_design_fsk(*bad, fp(a), fp(b)) == sr.ARGUMENT_ERROR, bad
        with pytest.raises(ValueError):
            sr.fsk_bandpass(*bad)
    assert not a.any() and not b.any()


def test_design_ita2_against_ita2_table_and_the_encoder():
    L = sr.lib()
    assert L.selenite_rx_design_ita2(None) == sr.ARGUMENT_ERROR
    t = np.full(64, 1, np.uint8)
    assert L.selenite_rx_design_ita2(t.ctypes.data_as(sr.u8p)) == 0
    assert t.tobytes() == sr.ita2_table().tobytes() == fo.table().tobytes()
    assert [i for i in range(64) if t[i] == 0] == [0, 27, 31, 32, 59, 63]                # NUL, FIGS, LTRS in both cases
    assert bytes(t[[1, 3, 4, 25, 32 + 1, 32 + 5, 32 + 9, 32 + 22]]) == b"EA B3\a$0"
    assert t[4] == t[36] == ord(" ") and t[8] == t[40] == ord("\r") and t[2] == t[34] == ord("\n")
    # every printing character has one code per case, and encode() finds it
    for case in (t[:32], t[32:]):
        p = case[case != 0]
        assert len(set(p.tolist())) == len(p) == 29
    for i in range(64):
        if t[i] and chr(t[i]) not in " \r\n":
            codes = fo.encode(chr(t[i]))
            assert codes[-1] == i % 32 and (codes[:-1] == [27]) == (i >= 32), i
