"""The keyer kernel's law code (selenite-lite_amd/csrc/tx_keyer_law.h) compiled for the host and held against the oracle: keyer_sample is the
sample form, keyer_tile the run-length form over 64-bit masks that k_tx_keyer runs with wave-uniform values.  No GPU: the header is plain
integer C++.  Bit-exact key bytes and state words, for every mode, units shorter and longer than a tile, and tiles of every length."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import rxcommon as rc
import txkeyer_oracle as ko

SRC = r"""
#include <stdint.h>
#include "tx_keyer_law.h"
using namespace srx;
// tile = 0: keyer_sample for every sample; else keyer_tile over tiles of `tile` samples (<= 64), masks built as the kernel builds them
extern "C" void keyer_host_run(uint32_t *words, const uint8_t *pad, uint32_t n, uint8_t *key, uint32_t u, uint32_t mode,
                               const uint8_t *text, const uint8_t *codes, uint32_t ring, uint32_t tile)
{
    KeyerState k{ words[0], words[1], words[2], words[3], words[4], words[5], words[6], words[7], words[8], words[9], words[10] };
    const KeyerText t{ text, codes, ring };
    auto bits = [&](uint32_t p, uint32_t &d, uint32_t &h, uint32_t &s) {
        d = p & 1u; h = (p >> 1) & 1u; s = (p >> 2) & 1u;
        if (mode == 0u) { s |= d | h; d = 0u; h = 0u; }
    };
    if (tile == 0) {
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t d, h, s;
            bits(pad[i], d, h, s);
            key[i] = (uint8_t)(keyer_sample(k, d, h, s, u, mode, t) | s);
        }
    } else {
        for (uint32_t n0 = 0; n0 < n; n0 += tile) {
            const uint32_t nv = n - n0 < tile ? n - n0 : tile;
            uint64_t D = 0, H = 0, S = 0;
            for (uint32_t i = 0; i < nv; ++i) {
                uint32_t d, h, s;
                bits(pad[n0 + i], d, h, s);
                D |= (uint64_t)d << i; H |= (uint64_t)h << i; S |= (uint64_t)s << i;
            }
            const uint64_t K = keyer_tile(k, D, H, S, nv, u, mode, t) | S;
            for (uint32_t i = 0; i < nv; ++i) key[n0 + i] = (uint8_t)((K >> i) & 1u);
        }
    }
    const uint32_t out[11] = { k.phase, k.left, k.last, k.dit_mem, k.dah_mem, k.squeeze, k.code, k.tgap, k.tail, k.head, k.skipped };
    for (int i = 0; i < 11; ++i) words[i] = out[i];
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    d = tmp_path_factory.mktemp("keyer_law")
    (d / "law.cpp").write_text(SRC)
    so = d / "law.so"
    subprocess.run([cxx, "-O1", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(rc.ROOT, "selenite-lite_amd", "csrc"), str(d / "law.cpp"), "-o", str(so)],
                   check=True)
    L = C.CDLL(str(so))
    L.keyer_host_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.keyer_host_run.restype = None
    return L


def host_run(L, k, pad, tile):
    """runs oracle channel `k`'s state through the C++ law; returns (key, words)"""
    words = np.array([getattr(k, w) for w in ko.WORDS], np.uint32)
    pad = np.ascontiguousarray(pad, np.uint8)
    key = np.zeros(len(pad), np.uint8)
    text, codes = np.ascontiguousarray(k.text), np.ascontiguousarray(k.codes)
    L.keyer_host_run(words.ctypes.data, pad.ctypes.data, len(pad), key.ctypes.data, k.unit, k.mode, text.ctypes.data, codes.ctypes.data, k.ring, tile)
    return key, dict(zip(ko.WORDS, (int(x) for x in words)))


@pytest.mark.parametrize("mode", [ko.STRAIGHT, ko.IAMBIC_A, ko.IAMBIC_B])
@pytest.mark.parametrize("unit", [1, 2, 7, 63, 64, 65, 200])
def test_sample_and_tile_forms_equal_the_oracle(host, mode, unit):
    rng = np.random.default_rng(1000 * mode + unit)
    texts = ["", "E", "AB C", "x  Y", " K~k ", "5 ="]
    for trial in range(12):
        n = int(rng.integers(1, 30 * unit + 70))
        k = ko.Keyer(mode, unit, 16)
        k.send(texts[trial % len(texts)])
        pad = ko.random_paddles(rng, 1, n, unit, p_idle=0.95 if trial % 3 == 0 else 0.5)[0]
        if trial % 4 == 1:                       # edges on the first and last sample of tiles
            for e in range(63, n - 1, 64):
                pad[e], pad[e + 1] = rng.integers(0, 8), rng.integers(0, 8)
        for tile in (0, 64, 24, 1, int(rng.integers(2, 64))):
            want = k.copy()
            wkey = want.run(pad)
            got, words = host_run(host, k, pad, tile)
            assert np.array_equal(got, wkey), (trial, tile, np.flatnonzero(got != wkey)[:4])
            assert words == want.words(), (trial, tile)


def test_states_that_only_a_state_view_can_set(host):
    """left != 0 while IDLE, memories set while IDLE, last > 1, code = 0: the law says what happens, and both forms follow it"""
    rng = np.random.default_rng(5)
    for trial in range(60):
        unit = int(rng.choice([1, 3, 64, 90]))
        k = ko.Keyer(int(rng.integers(0, 3)), unit, 8)
        k.send("AN")
        k.set_words(dict(phase=int(rng.integers(0, 3)), left=int(rng.choice([0, 1, 5, 70, 300])), last=int(rng.integers(0, 3)),
                         dit_mem=int(rng.integers(0, 2)), dah_mem=int(rng.integers(0, 2)), squeeze=int(rng.integers(0, 2)),
                         code=int(rng.choice([0, 1, 2, 5, 0b1101010])), tgap=int(rng.choice([0, 0, 2, 6]))))
        pad = ko.random_paddles(rng, 1, 260, unit, p_idle=0.8)[0]
        want = k.copy()
        wkey = want.run(pad)
        for tile in (0, 64):
            got, words = host_run(host, k, pad, tile)
            assert np.array_equal(got, wkey) and words == want.words(), (trial, tile)
