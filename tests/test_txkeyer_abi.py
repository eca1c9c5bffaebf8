"""CPU: the keyer's C-ABI (include/selenite_tx_keyer.h) -- what the header declares is what the library exports and the Python face binds;
struct layouts; the two host-only helpers."""
import os
import re
import subprocess

import numpy as np

import rxcommon as rc
import selenite_rx as sr
import txkeyer_oracle as ko

# name -> number of arguments
NAMES = {
    "selenite_tx_set_keyer": 2, "selenite_tx_keyer_send": 6, "selenite_tx_keyer_pending": 2,
    "selenite_tx_process_paddles_f32_device": 5, "selenite_tx_process_paddles_q15_device": 5,
    "selenite_tx_process_paddles_f32": 5, "selenite_tx_process_paddles_q15": 5,
    "selenite_tx_keyer_run_device": 4, "selenite_tx_keyer_key_device": 1,
    "selenite_tx_get_keyer_state": 2, "selenite_tx_set_keyer_state": 2, "selenite_tx_time_keyer_stage_device": 5,
    "selenite_tx_design_morse_codes": 2, "selenite_tx_keyer_unit": 2,
}


def declared(header):
    text = open(os.path.join(rc.ROOT, "include", header)).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(selenite_tx_[a-z0-9_]+)\s*\(", code)))


def test_symbols_exported_and_bound():
    L = sr.lib()
    assert declared("selenite_tx_keyer.h") == sorted(NAMES) == sorted(sr.TXKEYER_ABI_SYMBOLS)
    for n, nargs in NAMES.items():
        assert hasattr(L, n), n
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == nargs, n
    assert '#include "selenite_tx_keyer.h"' in open(os.path.join(rc.ROOT, "include", "selenite_tx.h")).read()      # one header to include
    for m in ("set_keyer", "clear_keyer", "keyer_send", "keyer_pending", "process_paddles", "process_paddles_host", "keyer_run",
              "keyer_key_device", "keyer_state", "set_keyer_state", "time_keyer_stage"):
        assert callable(getattr(sr.Tx, m))
    assert callable(sr.morse_codes) and callable(sr.keyer_unit)
    assert (sr.KEYER_STRAIGHT, sr.KEYER_IAMBIC_A, sr.KEYER_IAMBIC_B) == (0, 1, 2) and (sr.PADDLE_DIT, sr.PADDLE_DAH, sr.PADDLE_KEY) == (1, 2, 4)
    assert "TXKEYER_ABI_SYMBOLS" in open(os.path.join(rc.ROOT, "__graft_entry__.py")).read()


def test_the_older_headers_declare_what_they_declared():
    assert declared("selenite_tx.h") == sorted(sr.TX_ABI_SYMBOLS) and len(sr.TX_ABI_SYMBOLS) == 16
    assert declared("selenite_tx_cw.h") == sorted(sr.TXCW_ABI_SYMBOLS) and declared("selenite_tx_in.h") == sorted(sr.TXIN_ABI_SYMBOLS)
    assert declared("selenite_tx_fm.h") == sorted(sr.TXFM_ABI_SYMBOLS)
    others = set(sr.ABI_SYMBOLS) | set(sr.RING_ABI_SYMBOLS) | set(sr.TX_ABI_SYMBOLS) | set(sr.TXFM_ABI_SYMBOLS) | set(sr.TXCW_ABI_SYMBOLS) | \
        set(sr.TXIN_ABI_SYMBOLS) | set(sr.CHAN_ABI_SYMBOLS) | set(sr.COMB_ABI_SYMBOLS)
    assert not set(NAMES) & others


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_tx.h"
#define O(f) offsetof(selenite_tx_keyer_config, f)
#define V(f) offsetof(selenite_tx_keyer_state_view, f)
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_tx_keyer_config), O(struct_size), O(mode), O(unit_all), O(unit), O(ring), O(codes), O(reserved));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_tx_keyer_state_view), V(phase), V(left), V(last), V(dit_mem),
           V(dah_mem), V(squeeze), V(code), V(tgap), V(tail), V(head), V(skipped), V(text));
    printf("%d %d %d %d %d %d\n", SELENITE_KEYER_STRAIGHT, SELENITE_KEYER_IAMBIC_A, SELENITE_KEYER_IAMBIC_B, SELENITE_KEYER_DIT, SELENITE_KEYER_DAH,
           SELENITE_KEYER_KEY);
    return 0;
}
"""


def test_struct_layouts_match_the_header_in_plain_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(C_SNIPPET)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(rc.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    cfg, view, enums = (list(map(int, ln.split())) for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    K = sr.TxKeyerConfig
    assert cfg == [C_sizeof(K)] + [getattr(K, f).offset for f in ("struct_size", "mode", "unit_all", "unit", "ring", "codes", "reserved")]
    assert cfg[0] == 48
    W = sr.TxKeyerStateView
    assert view == [C_sizeof(W)] + [getattr(W, f).offset for f in sr.KEYER_STATE_WORDS + ("text",)] and view[0] == 96
    assert tuple(sr.KEYER_STATE_WORDS) == tuple(ko.WORDS)
    assert enums == [0, 1, 2, 1, 2, 4]


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def test_morse_codes_inverts_morse_table():
    table, codes = sr.morse_table(), sr.morse_codes()
    assert codes.dtype == np.uint8 and codes.shape == (256,)
    have = [c for c in range(2, 256) if table[c] != table[0]]
    assert len(have) == 26 + 10 + 8
    for code in have:                            # every character that has a pattern: its smallest one, which is this one (the table has no doubles)
        assert codes[table[code]] == code and table[codes[table[code]]] == table[code]
    for ch in range(ord("a"), ord("z") + 1):
        assert codes[ch] == codes[ch - 32] != 0
    assert codes[ord(" ")] == 1 and codes[table[0]] == 0
    named = {int(table[c]) for c in have} | set(range(ord("a"), ord("z") + 1)) | {ord(" ")}
    assert all(codes[c] == 0 for c in range(256) if c not in named)
    assert np.array_equal(codes, ko.builtin_codes()), "the oracle's own table"
    # another table: a character with two patterns takes the smaller, the filler none
    t2 = np.full(256, ord("?"), np.uint8)
    t2[5], t2[9], t2[0b110] = ord("x"), ord("x"), ord("?")
    c2 = sr.morse_codes(t2)
    assert c2[ord("x")] == 5 and c2[ord("?")] == 0 and c2[ord(" ")] == 1 and c2[ord("X")] == 0
    assert np.array_equal(sr.morse_codes(table), codes)
    assert sr.lib().selenite_tx_design_morse_codes(None, None) == sr.ARGUMENT_ERROR


def test_keyer_unit():
    assert sr.keyer_unit(20, 12000) == 720
    assert sr.keyer_unit(12, 12000) == 1200 and sr.keyer_unit(40, 12000) == 360 and sr.keyer_unit(25, 8000) == 384
    assert sr.keyer_unit(1e9, 12000) == 1 and sr.keyer_unit(0, 12000) == 0 and sr.keyer_unit(20, float("nan")) == 0
