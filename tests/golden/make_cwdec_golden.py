"""Writes tests/golden/cwdec.npz: three channels x 420 DSP blocks of n = 24 samples of keyed, noisy audio through the Morse decoder's law
(DESIGN.md section 2 step 4-d), for the numpy restatement in tests/cwdec_oracle.py (tests/test_cwdec_oracle.py checks it bit for bit against
this file) and for the library (tests/test_gpu_cwdec.py).  The power of every block is the reference's own arm_power_f32 (CMSIS-DSP 1.5.3);
the scalar law behind it is stated once more below, in C, independently of the restatement.  The file holds the audio, the lengths of the
calls, pw and ms of every block, and every row of the state behind every call.

The reference file (StatisticsFunctions/arm_power_f32.c) and the harness below are compiled into a temporary directory with oracle/Makefile's
flags (-std=gnu11 -O2 -ffp-contract=off -DARM_MATH_CM4), run, and deleted: nothing compiled is kept, and no test or build step compiles
reference code.  Run by hand where the reference tree is:
    python3 tests/golden/make_cwdec_golden.py REFERENCE_ROOT      (the root of the reference firmware tree)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cwdec.npz")

HARNESS = r"""
#include <float.h>
#include "arm_math.h"
typedef struct {
    float peak_attack, peak_decay, floor_attack, floor_decay, on_frac, off_frac, snr, min_power;
    uint32_t debounce, adapt, track, unit_min, unit_max, ring;
} cw_par;
typedef struct {
    float peak, floor;
    uint32_t primed, key, flip, run, unit, code, word;
    uint64_t count;
} cw_state;
static void emit(cw_state *s, uint8_t *text, uint32_t ring, uint8_t c) { text[s->count % ring] = c; s->count += 1; }
/* x [nblocks][n] of one channel; pw, ms [nblocks]; s and text [ring] run on from call to call */
void cwdec_run(const cw_par *p, const uint8_t *table, int n, int nblocks, const float *x, cw_state *s, uint8_t *text, float *pw, float *ms_out)
{
    for (int b = 0; b < nblocks; ++b) {
        float ms, r, d, t, span, f, thr, q;
        uint32_t raw = 0, edge = 0, ended = 0;
        arm_power_f32((float *)x + (size_t)b * n, (uint32_t)n, pw + b);
        ms = pw[b] / (float)n;
        ms_out[b] = ms;
        if (ms <= FLT_MAX) {
            if (!s->primed) { s->peak = ms; s->floor = ms; s->primed = 1; }
            else {
                r = ms > s->peak ? p->peak_attack : p->peak_decay;    d = ms - s->peak;   t = r * d;  s->peak = s->peak + t;
                r = ms < s->floor ? p->floor_attack : p->floor_decay; d = ms - s->floor;  t = r * d;  s->floor = s->floor + t;
            }
            span = s->peak - s->floor;  f = s->key ? p->off_frac : p->on_frac;  t = f * span;  thr = s->floor + t;
            q = p->snr * s->floor;
            raw = (s->peak > q && s->peak > p->min_power) && ms > thr;
        }
        if (raw == s->key) { s->run = s->run + s->flip + 1 < 65535 ? s->run + s->flip + 1 : 65535; s->flip = 0; }
        else { s->flip += 1;  if (s->flip >= p->debounce) { ended = s->run; s->key = raw; s->run = s->flip; s->flip = 0; edge = 1; } }
        if (edge && s->key == 0) {
            uint32_t m = ended << 8, dah = m >= 2 * s->unit;
            if (p->adapt) {
                uint32_t g = dah ? m / 3 : m;
                if (g >= s->unit) s->unit += (g - s->unit) >> p->track; else s->unit -= (s->unit - g) >> p->track;
                if (s->unit < p->unit_min) s->unit = p->unit_min;
                if (s->unit > p->unit_max) s->unit = p->unit_max;
            }
            s->code = (s->code == 0 || s->code >= 128) ? 0 : (s->code << 1) | dah;
        }
        if (s->key == 0) {
            uint32_t sp = s->run << 8;
            if (s->code != 1 && sp >= 2 * s->unit) { emit(s, text, p->ring, table[s->code]); s->code = 1; s->word = 1; }
            if (s->word && sp >= 5 * s->unit) { emit(s, text, p->ring, ' '); s->word = 0; }
        }
    }
}
"""


class Par(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("peak_attack", "peak_decay", "floor_attack", "floor_decay", "on_frac", "off_frac", "snr", "min_power")] + \
               [(k, C.c_uint32) for k in ("debounce", "adapt", "track", "unit_min", "unit_max", "ring")]


class State(C.Structure):
    _fields_ = [("peak", C.c_float), ("floor", C.c_float)] + [(k, C.c_uint32) for k in ("primed", "key", "flip", "run", "unit", "code", "word")] + \
               [("count", C.c_uint64)]


MORSE = {"C": "-.-.", "Q": "--.-", "K": "-.-", "5": ".....", "N": "-.", "T": "-", "U": "..-"}      # what the fixture sends
N, BLOCKS, CHANNELS = 24, 420, 3
LENS = (1, 65, 7, 3, 130, 64, 16, 2, 32, 100)                       # DSP blocks per call: 420 in all; calls 2 - 5 end inside a debounce (flip = 1)
PAR = dict(peak_attack=0.5, peak_decay=0.002, floor_attack=0.25, floor_decay=0.002, on_frac=0.4, off_frac=0.25, snr=4.0, min_power=1e-8,
           debounce=2, adapt=1, track=2, unit_min=2 * 256, unit_init=6 * 256, unit_max=64 * 256, ring=16)
SENT = (("CQ K", 5), ("5NN TU", 7))                               # text and dit length in DSP blocks of channels 0 and 1; channel 2: noise
ROWS = dict(peak=np.float32, floor=np.float32, primed=np.uint32, key=np.uint32, flip=np.uint32, run=np.uint32, unit=np.uint32, code=np.uint32,
            word=np.uint32, count=np.uint64)


def key_of(text, unit):
    out = []
    for w, word in enumerate(text.split()):
        if w:
            out.append(np.zeros(7 * unit))
        for c, ch in enumerate(word):
            if c:
                out.append(np.zeros(3 * unit))
            for e, el in enumerate(MORSE[ch]):
                if e:
                    out.append(np.zeros(unit))
                out.append(np.ones((3 if el == "-" else 1) * unit))
    return np.concatenate(out)


def make_audio():
    rng = np.random.default_rng(0x43574445)
    total = N * BLOCKS
    x = rng.uniform(-0.03, 0.03, (CHANNELS, total))
    t = np.arange(total)
    w = np.hanning(31)
    w /= w.sum()
    for c, (text, unit_blocks) in enumerate(SENT):
        key = np.zeros(total)
        k = key_of(text, unit_blocks * N)
        lead = (20 + 3 * c) * N + 5 * c                             # (edges off the block grid)
        assert lead + len(k) + 5 * unit_blocks * N < total, (c, lead + len(k), total)
        key[lead:lead + len(k)] = k
        x[c] += 0.1 * np.convolve(key, w, mode="same") * np.sin(2 * np.pi * t / 20.0)
    x = x.astype(np.float32)
    x[2, 100 * N + 7] = np.nan                                      # a NaN block and an Inf block in the noise channel
    x[2, 300 * N + 11] = np.inf
    x[2, 200 * N:230 * N] *= np.float32(8.0)                        # ... and a burst that opens and closes its key
    return x


def table():
    t = np.full(256, ord("#"), np.uint8)
    for ch, pat in MORSE.items():
        code = 1
        for e in pat:
            code = (code << 1) | (e == "-")
        t[code] = ord(ch)
    return t


def main(ref_root):
    dsp = os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Source")
    inc = ["-I" + os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Include"), "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Core", "Include"),
           "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Include")]
    srcs = [os.path.join(dsp, "StatisticsFunctions", "arm_power_f32.c")]
    x, tab = make_audio(), table()
    out = dict(x=x, lens=np.array(LENS, np.int64), n=np.int64(N), table=tab, sent=np.array([s for s, _ in SENT]))
    for k, v in PAR.items():
        out["par/" + k] = np.float32(v) if isinstance(v, float) else np.int64(v)
    calls = {k: np.zeros((len(LENS), CHANNELS), t) for k, t in ROWS.items()}
    calls["text"] = np.zeros((len(LENS), CHANNELS, PAR["ring"]), np.uint8)
    pw, ms = np.zeros((CHANNELS, BLOCKS), np.float32), np.zeros((CHANNELS, BLOCKS), np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        h = os.path.join(tmp, "harness.c")
        with open(h, "w") as f:
            f.write(HARNESS)
        so = os.path.join(tmp, "libcwdec.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-w", "-DARM_MATH_CM4"] + inc + ["-shared", "-o", so, h] + srcs
                       + ["-lm"], check=True)
        L = C.CDLL(so)
        fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        L.cwdec_run.argtypes = [C.POINTER(Par), bp, C.c_int, C.c_int, fp, C.POINTER(State), bp, fp, fp]
        par = Par(**{k: v for k, v in PAR.items() if k != "unit_init"})
        for c in range(CHANNELS):
            st, text, at = State(unit=PAR["unit_init"], code=1), np.zeros(PAR["ring"], np.uint8), 0
            for i, nb in enumerate(LENS):
                xs = np.ascontiguousarray(x[c, at * N:(at + nb) * N])
                p, m = np.zeros(nb, np.float32), np.zeros(nb, np.float32)
                L.cwdec_run(C.byref(par), tab.ctypes.data_as(bp), N, nb, xs.ctypes.data_as(fp), C.byref(st), text.ctypes.data_as(bp),
                            p.ctypes.data_as(fp), m.ctypes.data_as(fp))
                pw[c, at:at + nb], ms[c, at:at + nb] = p, m
                at += nb
                for k in ROWS:
                    calls[k][i, c] = getattr(st, k)
                calls["text"][i, c] = text
            got = text[:st.count].tobytes().decode()
            print("channel %d: %r, unit %.2f blocks" % (c, got, st.unit / 256.0))
            if c < len(SENT):
                assert got.rstrip() == SENT[c][0], (got, SENT[c][0])
    assert np.isnan(ms[2, 100]) and np.isinf(ms[2, 300]) and calls["key"].any()
    out["pw"], out["ms"] = pw, ms
    for k, v in calls.items():
        out["call/" + k] = v
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
