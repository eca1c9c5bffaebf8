"""Writes tests/golden/out_stage.npz: arm_fir_interpolate_f32 and arm_float_to_q15 (both builds) of the reference's CMSIS-DSP 1.5.3, run on
seeded input, for the restatement of the audio output stage in tests/out_oracle.py (tests/test_out_oracle.py checks it bit for bit against
this file).

The reference files (FilteringFunctions/arm_fir_interpolate_f32.c, arm_fir_interpolate_init_f32.c, SupportFunctions/arm_float_to_q15.c --
the latter twice, as the firmware builds it and with ARM_MATH_ROUNDING) and the small harness below are compiled into a temporary
directory with oracle/Makefile's flags (-std=gnu11 -O2 -ffp-contract=off -DARM_MATH_CM4), run, and deleted: nothing compiled is kept, and
no test or build step compiles reference code.

arm_float_to_q15 casts in * 32768 to q31_t (arm_float_to_q15.c:117): outside the int32 range that cast is undefined in C -- this build gives
INT_MIN for either sign where the firmware's FPU (and the GPU's v_cvt_i32_f32) saturates by sign, the behaviour oracle/rx_oracle.c states.
The int16 words are recorded everywhere; `q_defined` marks the samples whose cast is defined (all of them at levels 1e-22 and 1, next to
none at 1e18), and the test compares the reference's words there and asks for saturation by sign everywhere else.  Run by hand where the reference tree is:
    python3 tests/golden/make_out_golden.py REFERENCE_ROOT      (the root of the reference firmware tree)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "out_stage.npz")

# our harness: one instance per case, the input cut into calls of the given lengths (state carried by the instance)
HARNESS = r"""
#include "arm_math.h"
#include <stdlib.h>
#include <string.h>
void arm_float_to_q15_rounding(float32_t *pSrc, q15_t *pDst, uint32_t blockSize);
int out_run(int L, int num_taps, const float *coeffs, const float *src, int ncalls, const int *lens, float *dst, float *state_final,
            int16_t *q_trunc, int16_t *q_round)
{
    int total = 0, maxlen = 0;
    for (int i = 0; i < ncalls; ++i) { total += lens[i]; if (lens[i] > maxlen) maxlen = lens[i]; }
    const int P = num_taps / L;
    float *state = (float *)malloc(sizeof(float) * (P + maxlen - 1));
    arm_fir_interpolate_instance_f32 S;
    if (arm_fir_interpolate_init_f32(&S, (uint8_t)L, (uint16_t)num_taps, (float32_t *)coeffs, state, (uint32_t)maxlen) != ARM_MATH_SUCCESS) return -1;
    int at = 0;
    for (int i = 0; i < ncalls; ++i) {
        arm_fir_interpolate_f32(&S, (float32_t *)src + at, dst + (size_t)at * L, (uint32_t)lens[i]);
        at += lens[i];
    }
    memcpy(state_final, state, sizeof(float) * (P - 1));
    arm_float_to_q15(dst, q_trunc, (uint32_t)(total * L));
    arm_float_to_q15_rounding(dst, q_round, (uint32_t)(total * L));
    free(state);
    return total;
}
"""

INTERPS = (1, 2, 4, 8)
PHASES = (1, 3, 8, 13, 64)
LEVELS = (1e-22, 1.0, 1e18)
# the stream (192 samples) in DSP blocks of 24, of 64, as one call, and as six uneven calls (some shorter than the history)
CUTS = {"b24": [24] * 8, "b64": [64] * 3, "one": [192], "uneven": [1, 7, 64, 100, 3, 17]}
TOTAL = 192
SEED = 0x4F5554


def main(ref_root):
    dsp = os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Source")
    inc = ["-I" + os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Include"), "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Core", "Include"),
           "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Include")]
    flags = ["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-w", "-DARM_MATH_CM4"] + inc
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        h = os.path.join(tmp, "harness.c")
        with open(h, "w") as f:
            f.write(HARNESS)
        q15 = os.path.join(dsp, "SupportFunctions", "arm_float_to_q15.c")
        o_round = os.path.join(tmp, "q15_round.o")
        subprocess.run(flags + ["-DARM_MATH_ROUNDING", "-Darm_float_to_q15=arm_float_to_q15_rounding", "-c", "-o", o_round, q15], check=True)
        so = os.path.join(tmp, "libout.so")
        subprocess.run(flags + ["-shared", "-o", so, h, o_round, q15, os.path.join(dsp, "FilteringFunctions", "arm_fir_interpolate_f32.c"),
                                os.path.join(dsp, "FilteringFunctions", "arm_fir_interpolate_init_f32.c")], check=True)
        L = C.CDLL(so)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int16)
        L.out_run.argtypes = [C.c_int, C.c_int, fp, fp, C.c_int, C.POINTER(C.c_int), fp, fp, ip, ip]
        rng = np.random.default_rng(SEED)
        t = np.arange(TOTAL)
        names = []
        for li, interp in enumerate(INTERPS):
            for pi, plen in enumerate(PHASES):
                nt = interp * plen
                coeffs = (2.0 * rng.standard_normal(nt) / np.sqrt(plen)).astype(np.float32)     # output rms ~1.4 at level 1: arm_float_to_q15 saturates
                for level in LEVELS:
                    # a tone plus noise, peaks above 1 at level 1 (arm_float_to_q15 saturates both ways there)
                    x = ((0.9 * np.sin(2 * np.pi * 0.031 * t + li + pi) + 0.3 * rng.standard_normal(TOTAL)) * level).astype(np.float32)
                    name = "L%d_P%d_lvl%g" % (interp, plen, level)
                    names.append(name)
                    out[name + "/interp"], out[name + "/coeffs"], out[name + "/src"] = np.int32(interp), coeffs, x
                    first = None
                    for cut, lens in CUTS.items():
                        assert sum(lens) == TOTAL
                        y, st = np.empty(TOTAL * interp, np.float32), np.empty(max(plen - 1, 0), np.float32)
                        qt, qr = np.empty(TOTAL * interp, np.int16), np.empty(TOTAL * interp, np.int16)
                        lens_a = (C.c_int * len(lens))(*lens)
                        p = lambda a: a.ctypes.data_as(fp)  # noqa: E731
                        rc = L.out_run(interp, nt, p(coeffs), p(x), len(lens), lens_a, p(y), p(st), qt.ctypes.data_as(ip), qr.ctypes.data_as(ip))
                        assert rc == TOTAL, (name, cut, rc)
                        if first is None:       # the reference's bits do not depend on the cut: one copy is kept, the others are checked here
                            first = (y, st, qt, qr)
                            out[name + "/y"], out[name + "/state"], out[name + "/q_trunc"], out[name + "/q_round"] = y, st, qt, qr
                            out[name + "/q_defined"] = np.abs(y.astype(np.float64)) * 32768.0 + 1.0 < 2147483648.0
                        else:
                            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, (y, st, qt, qr))), (name, cut)
    out["cases"] = np.array(names)
    out["cut_names"] = np.array(list(CUTS))
    for cut, lens in CUTS.items():
        out["cut/" + cut] = np.asarray(lens, np.int32)
    out["seed"] = np.int64(SEED)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
