"""Writes tests/golden/fskdec.npz: four channels x 900 ticks of T = 8 samples of FSK-keyed, noisy audio through the FSK teleprinter decoder's
law, for the numpy restatement in tests/fskdec_oracle.py (tests/test_fskdec_oracle.py checks it bit for bit
against this file) and for the library (tests/test_gpu_fskdec.py).  The two tone filters are the reference's own
arm_biquad_cascade_df1_f32 with one section each and the three powers its arm_power_f32 (CMSIS-DSP 1.5.3); the scalar law behind them is
stated once more below, in C, independently of the restatement.  The file holds the audio, the lengths of the calls, pm, ps, pw and the
filter state behind every tick, and every row of the state behind every call.

The reference files (FilteringFunctions/arm_biquad_cascade_df1_f32.c, StatisticsFunctions/arm_power_f32.c) and the harness below are
compiled into a temporary directory with oracle/Makefile's flags (-std=gnu11 -O2 -ffp-contract=off -DARM_MATH_CM4), run, and deleted: nothing compiled is kept, and no test or build step compiles reference code.  Run by
hand where the reference tree is:
    python3 tests/golden/make_fskdec_golden.py REFERENCE_ROOT      (the root of the reference firmware tree)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "fskdec.npz")

HARNESS = r"""
#include <float.h>
#include "arm_math.h"
typedef struct { float alpha, hyst, frac, min_power; uint32_t reverse, usos, ring; } fsk_par;
typedef struct {
    float filt[8];                  /* mark {x1, x2, y1, y2}, space {x1, x2, y1, y2}: the two instances' pState */
    float em, es, ew;
    uint32_t lvl, k, t_q8, shift, figs, ferr, bit;
    uint64_t count;
} fsk_state;
enum { IDLE = 0, START = 1, STOP = 7 };
static void put(fsk_state *s, uint8_t *text, uint32_t ring, uint8_t b) { if (b) { text[s->count % ring] = b; s->count += 1; } }
static void follow(float *e, float v, float alpha) { float d = v - *e; float t = alpha * d; *e = *e + t; }
/* x [ticks][T] of one channel; pm, ps, pw [ticks] as measured (before `reverse`); trace [ticks][8] the filter state behind every tick;
 * s and text [ring] run on from call to call */
void fskdec_run(const fsk_par *p, const float *mark, const float *space, const uint8_t *table, int T, int ticks, const float *x, fsk_state *s,
                uint8_t *text, float *pm_out, float *ps_out, float *pw_out, float *trace)
{
    arm_biquad_casd_df1_inst_f32 fm, fs;
    float ym[256], ys[256];
    /* what arm_biquad_cascade_df1_init_f32 sets, less its clearing of pState: the state runs on from call to call */
    fm.numStages = 1; fm.pCoeffs = (float *)mark; fm.pState = s->filt;
    fs.numStages = 1; fs.pCoeffs = (float *)space; fs.pState = s->filt + 4;
    for (int i = 0; i < ticks; ++i) {
        float pm, ps, pw, tot, diff;
        uint32_t was, level, present;
        const float *xi = x + (size_t)i * T;
        arm_biquad_cascade_df1_f32(&fm, (float *)xi, ym, (uint32_t)T);
        arm_biquad_cascade_df1_f32(&fs, (float *)xi, ys, (uint32_t)T);
        arm_power_f32(ym, (uint32_t)T, &pm);
        arm_power_f32(ys, (uint32_t)T, &ps);
        arm_power_f32((float *)xi, (uint32_t)T, &pw);
        pm_out[i] = pm; ps_out[i] = ps; pw_out[i] = pw;
        for (int j = 0; j < 8; ++j) trace[(size_t)i * 8 + j] = s->filt[j];
        if (p->reverse) { float t = pm; pm = ps; ps = t; }
        if (pm <= FLT_MAX && ps <= FLT_MAX && pw <= FLT_MAX) { follow(&s->em, pm, p->alpha); follow(&s->es, ps, p->alpha); follow(&s->ew, pw, p->alpha); }
        tot = s->em + s->es;
        diff = s->em - s->es;
        present = tot > p->frac * s->ew && tot > p->min_power && tot <= FLT_MAX;
        was = s->lvl;
        level = was;
        if (!present || diff > p->hyst * tot) level = 1;
        else if (-diff > p->hyst * tot) level = 0;
        s->lvl = level;
        if (s->k == IDLE) {
            if (was == 1 && level == 0) { s->k = START; s->t_q8 = 0; s->shift = 0; }
            continue;
        }
        s->t_q8 += 256;
        if (s->t_q8 < (s->k - 1) * s->bit + s->bit / 2) continue;             /* not yet at the centre of this bit */
        switch (s->k) {
        case START:
            s->k = level ? IDLE : 2;
            break;
        case STOP:
            if (!level) s->ferr += 1;
            else if (s->shift == 31) s->figs = 0;
            else if (s->shift == 27) s->figs = 1;
            else {
                put(s, text, p->ring, table[s->figs * 32 + s->shift]);
                if (p->usos && s->shift == 4) s->figs = 0;
            }
            s->k = IDLE;
            break;
        default:                                                              /* data bits 0 .. 4 at k = 2 .. 6 */
            if (level) s->shift |= 1u << (s->k - 2);
            s->k += 1;
        }
    }
}
"""


class Par(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("alpha", "hyst", "frac", "min_power")] + [(k, C.c_uint32) for k in ("reverse", "usos", "ring")]


class State(C.Structure):
    _fields_ = [("filt", C.c_float * 8), ("em", C.c_float), ("es", C.c_float), ("ew", C.c_float)] + \
               [(k, C.c_uint32) for k in ("lvl", "k", "t_q8", "shift", "figs", "ferr", "bit")] + [("count", C.c_uint64)]


LETTERS = "\0E\nA SIU\rDRJNFCKTZLWHYPQOBG\0MXV\0"
FIGURES = "\0" "3\n- \a87\r$4',!:(5\")2#6019?&\0./;\0"
T, TICKS, CHANNELS = 8, 900, 4
LENS = (1, 130, 7, 3, 260, 64, 33, 2, 300, 100)                     # ticks per call: 900 in all
F_MARK, F_SPACE, BW = 0.15, 0.20, 0.02                              # cycles per sample
PAR = dict(tick=T, bit_q8=10 * 256, reverse=0, usos=1, ring=16, alpha=0.25, hyst=0.1, frac=0.35, min_power=1e-6)
# text and samples per bit of channels 0 - 2; channel 2 is hit by a NaN inside its fourth character; channel 3: noise with an Inf and a burst
SENT = (("RY 59 K", 80.0), ("DE W1AW (5)", 56.0), ("CQ CQ", 80.0))
ROWS = dict(em=np.float32, es=np.float32, ew=np.float32, lvl=np.uint32, k=np.uint32, t_q8=np.uint32, shift=np.uint32, figs=np.uint32,
            ferr=np.uint32, bit=np.uint32, count=np.uint64)


def table():
    return np.frombuffer((LETTERS + FIGURES).encode("latin-1"), np.uint8).copy()


def design(f0):
    w = 2.0 * np.pi * f0
    al = np.sin(w) / (2.0 * f0 / BW)
    return (np.array([al, 0.0, -al, 2.0 * np.cos(w), -(1.0 - al)]) / (1.0 + al)).astype(np.float32)


def encode(text):
    codes, figs = [], 0
    for ch in text:
        want = (FIGURES if figs else LETTERS).find(ch)
        if want < 0:
            figs ^= 1
            codes.append(27 if figs else 31)
            want = (FIGURES if figs else LETTERS).find(ch)
        assert want > 0, ch
        codes.append(want)
        if want == 4:
            figs = 0                                               # usos
    return codes


def keyed(codes, per_bit, lead):
    """phase-continuous tone pair: start (space), five data bits LSB first (1 = mark), 1.5 stop bits; `lead` bits of mark in front"""
    bits = [1.0] * lead
    for c in codes:
        bits += [0.0, 0.0] + [float((c >> b) & 1) for b in range(5) for _ in range(2)] + [1.0] * 3       # half bits
    half = per_bit / 2.0
    n = int(len(bits) * half)
    idx = np.minimum((np.arange(n) / half).astype(int), len(bits) - 1)
    f = np.where(np.array(bits)[idx] == 1.0, F_MARK, F_SPACE)
    return np.sin(2.0 * np.pi * np.cumsum(f))


def make_audio():
    rng = np.random.default_rng(0x46534B44)
    total = T * TICKS
    x = rng.normal(0.0, 0.05, (CHANNELS, total))
    for c, (text, per_bit) in enumerate(SENT):
        a = 0.3 * keyed(encode(text), per_bit, 12 + 2 * c)
        assert a.size + 4 * per_bit < total, (c, a.size, total)
        x[c, :a.size] += a
        x[c, a.size:] += 0.3 * np.sin(2.0 * np.pi * F_MARK * np.arange(a.size, total) + 1.0)      # (idle mark; the phase step is one glitch)
    x = x.astype(np.float32)
    x[2, int((8 + 3 * 7.5 + 3) * 80)] = np.nan                     # channel 2: 8 bits of lead, three characters, three bits into the fourth
    x[3, 300 * T + 5] = np.inf
    x[3, 500 * T:560 * T] += (0.4 * np.sin(2.0 * np.pi * F_SPACE * np.arange(60 * T))).astype(np.float32)      # a burst of space: a false start
    return x


def main(ref_root):
    dsp = os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Source")
    inc = ["-I" + os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Include"), "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Core", "Include"),
           "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Include")]
    srcs = [os.path.join(dsp, "FilteringFunctions", "arm_biquad_cascade_df1_f32.c"), os.path.join(dsp, "StatisticsFunctions", "arm_power_f32.c")]
    x, tab, mark, space = make_audio(), table(), design(F_MARK), design(F_SPACE)
    bits = np.array([int(round(per_bit / T * 256.0)) for _, per_bit in SENT] + [PAR["bit_q8"]], np.uint32)      # the `bit` row: per channel
    out = dict(x=x, lens=np.array(LENS, np.int64), table=tab, mark=mark, space=space, bit=bits, sent=np.array([s for s, _ in SENT]))
    for k, v in PAR.items():
        out["par/" + k] = np.float32(v) if isinstance(v, float) else np.int64(v)
    calls = {k: np.zeros((len(LENS), CHANNELS), t) for k, t in ROWS.items()}
    calls["filt"] = np.zeros((len(LENS), CHANNELS, 2, 4), np.float32)
    calls["text"] = np.zeros((len(LENS), CHANNELS, PAR["ring"]), np.uint8)
    pw = {k: np.zeros((CHANNELS, TICKS), np.float32) for k in ("pm", "ps", "pw")}
    trace = np.zeros((CHANNELS, TICKS, 2, 4), np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        h = os.path.join(tmp, "harness.c")
        with open(h, "w") as f:
            f.write(HARNESS)
        so = os.path.join(tmp, "libfskdec.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-w", "-DARM_MATH_CM4"] + inc + ["-shared", "-o", so, h] + srcs
                       + ["-lm"], check=True)
        L = C.CDLL(so)
        fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        L.fskdec_run.argtypes = [C.POINTER(Par), fp, fp, bp, C.c_int, C.c_int, fp, C.POINTER(State), bp, fp, fp, fp, fp]
        par = Par(**{k: PAR[k] for k in ("alpha", "hyst", "frac", "min_power", "reverse", "usos", "ring")})
        for c in range(CHANNELS):
            st, text, at = State(lvl=1, bit=int(bits[c])), np.zeros(PAR["ring"], np.uint8), 0
            for i, nt in enumerate(LENS):
                xs = np.ascontiguousarray(x[c, at * T:(at + nt) * T])
                p = [np.zeros(nt, np.float32) for _ in range(3)]
                tr = np.zeros((nt, 8), np.float32)
                L.fskdec_run(C.byref(par), mark.ctypes.data_as(fp), space.ctypes.data_as(fp), tab.ctypes.data_as(bp), T, nt, xs.ctypes.data_as(fp),
                             C.byref(st), text.ctypes.data_as(bp), p[0].ctypes.data_as(fp), p[1].ctypes.data_as(fp), p[2].ctypes.data_as(fp),
                             tr.ctypes.data_as(fp))
                for k, v in zip(("pm", "ps", "pw"), p):
                    pw[k][c, at:at + nt] = v
                trace[c, at:at + nt] = tr.reshape(nt, 2, 4)
                at += nt
                for k in ROWS:
                    calls[k][i, c] = getattr(st, k)
                calls["filt"][i, c] = np.array(st.filt[:], np.float32).reshape(2, 4)
                calls["text"][i, c] = text
            n = int(st.count)
            got = (text[:n] if n <= len(text) else np.concatenate([text[n % len(text):], text[:n % len(text)]])).tobytes().decode("latin-1")
            print("channel %d: count %d, ferr %d, last %r" % (c, n, st.ferr, got))
            if c == 2:
                # the followers froze where they stood and lvl with them: the running character ends on that level, then nothing is read
                assert got.startswith("CQ ") and n <= 4 and st.k == 0 and np.isnan(st.filt[2]) and np.isnan(st.filt[6]), got
            if c < 2:
                assert got == SENT[c][0][-len(got):] and n == len(SENT[c][0]) and st.ferr == 0, (got, SENT[c][0])
    assert np.isnan(pw["pw"][2]).any() and np.isinf(pw["pw"][3]).any() and (calls["lvl"] == 0).any() and (calls["k"] != 0).any()
    assert calls["count"][-1, 3] == 0
    out.update(pw)
    out["trace"] = trace
    for k, v in calls.items():
        out["call/" + k] = v
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
