"""Writes tests/golden/lms_norm.npz: arm_lms_norm_f32 of the reference's CMSIS-DSP 1.5.3, run on seeded input, for the numpy
restatement in tests/nr_oracle.py (tests/test_nr_oracle.py checks it bit for bit against this file).

The two reference files (FilteringFunctions/arm_lms_norm_f32.c, arm_lms_norm_init_f32.c) and the small harness below are compiled
into a temporary directory with oracle/Makefile's flags (-std=gnu11 -O2 -ffp-contract=off -DARM_MATH_CM4), run, and deleted:
nothing compiled is kept, and no test or build step compiles reference code.  Run by hand where the reference tree is:
    python3 tests/golden/make_nr_golden.py REFERENCE_ROOT      (the root of the reference firmware tree)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "lms_norm.npz")

# our harness: one instance per case, the input cut into calls of the given lengths (state carried by the instance)
HARNESS = r"""
#include "arm_math.h"
#include <stdlib.h>
#include <string.h>
int nr_run(int num_taps, float mu, const float *coeffs_init, const float *src, const float *ref, int ncalls, const int *lens,
           float *out, float *err, float *coeffs_final, float *window_final, float *energy_x0)
{
    int total = 0, maxlen = 0;
    for (int i = 0; i < ncalls; ++i) { total += lens[i]; if (lens[i] > maxlen) maxlen = lens[i]; }
    float *state = (float *)malloc(sizeof(float) * (num_taps + maxlen - 1));
    arm_lms_norm_instance_f32 S;
    memcpy(coeffs_final, coeffs_init, sizeof(float) * num_taps);
    arm_lms_norm_init_f32(&S, (uint16_t)num_taps, coeffs_final, state, mu, (uint32_t)maxlen);
    int at = 0;
    for (int i = 0; i < ncalls; ++i) {
        arm_lms_norm_f32(&S, (float32_t *)src + at, (float32_t *)ref + at, out + at, err + at, (uint32_t)lens[i]);
        at += lens[i];
    }
    memcpy(window_final, state, sizeof(float) * (num_taps - 1));
    energy_x0[0] = S.energy;
    energy_x0[1] = S.x0;
    free(state);
    return total;
}
"""

# (name, num_taps, mu, calls[, shaping]): one long call against seven uneven calls of the same samples; then (appended: every case draws from
# the one seeded stream, so the arrays of the cases before it stay what they were) the edges of the arithmetic --
#   ("gap", a, b, L): the signal, scaled by L, is exactly zero over samples a .. b - 1 -- a burst, silence, the signal back (the first edge inside a call, the
#                  second on a call boundary).  In the silence `energy` is what the roundings of energy -= x0*x0, += in*in left: negative here
#                  (tests/test_nr_oracle.py asserts it), so energy + eps is negative when the signal returns;
#   ("level", L):  the signal scaled by L -- 1e-22: in*in and `energy` are denormals; 1e18: energy ~ 1e37, still finite;
# and many calls shorter than the window (the copy-back of arm_lms_norm_f32.c:315-346 after one, two, three samples).
CASES = [("t5_mu0.5", 5, 0.5, [600]), ("t8_mu0.01", 8, 0.01, [600]), ("t16_mu0.5", 16, 0.5, [600]),
         ("t32_mu1.5", 32, 1.5, [600]), ("t64_mu0.5", 64, 0.5, [600]), ("t32_mu0.5_one", 32, 0.5, [1000]),
         ("t32_mu0.5_seven", 32, 0.5, [1, 7, 64, 129, 300, 3, 496]), ("t64_mu0.01_seven", 64, 0.01, [33, 5, 200, 62, 250, 1, 49]),
         ("t8_mu0.05_gap", 8, 0.05, [250, 200, 150, 400], ("gap", 300, 600, 1.0)),
         ("t64_mu1.5_gap", 64, 1.5, [250, 200, 150, 400], ("gap", 300, 600, 1.5)),
         ("t32_mu0.5_lvl1e-22", 32, 0.5, [500, 500], ("level", 1e-22)), ("t32_mu0.5_lvl1e18", 32, 0.5, [500, 500], ("level", 1e18)),
         ("t16_mu0.5_short", 16, 0.5, [1, 1, 2, 3, 12, 24, 5, 36, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 4, 60, 63, 64, 65, 2, 24, 24, 12, 48, 96, 1, 100, 23, 25, 61])]
SEED = 0x4C4D53


def main(ref_root):
    src_dir = os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Source", "FilteringFunctions")
    inc = ["-I" + os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Include"), "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Core", "Include"),
           "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Include")]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        h = os.path.join(tmp, "harness.c")
        with open(h, "w") as f:
            f.write(HARNESS)
        so = os.path.join(tmp, "liblms.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-w", "-DARM_MATH_CM4"] + inc +
                       ["-shared", "-o", so, h, os.path.join(src_dir, "arm_lms_norm_f32.c"), os.path.join(src_dir, "arm_lms_norm_init_f32.c")],
                       check=True)
        L = C.CDLL(so)
        fp = C.POINTER(C.c_float)
        L.nr_run.argtypes = [C.c_int, C.c_float, fp, fp, fp, C.c_int, C.POINTER(C.c_int), fp, fp, fp, fp, fp]
        rng = np.random.default_rng(SEED)
        for ci, (name, n, mu, lens, *shaping) in enumerate(CASES):
            total = sum(lens)
            t = np.arange(total + 64)
            # a tone plus noise; pSrc is pRef delayed by 3 samples (the stage's shape)
            x = (0.6 * np.sin(2 * np.pi * 0.031 * t + ci) + 0.2 * rng.standard_normal(total + 64)).astype(np.float32)
            if shaping and shaping[0][0] == "gap":
                x = x * np.float32(shaping[0][3])
                x[64 + shaping[0][1]:64 + shaping[0][2]] = 0.0
            if shaping and shaping[0][0] == "level":
                x = x * np.float32(shaping[0][1])
            ref, src = x[64:].copy(), x[61:61 + total].copy()
            init = (0.01 * rng.standard_normal(n)).astype(np.float32) if ci % 2 else np.zeros(n, np.float32)
            y, e = np.empty(total, np.float32), np.empty(total, np.float32)
            cf, win, ex = np.empty(n, np.float32), np.empty(n - 1, np.float32), np.empty(2, np.float32)
            lens_a = (C.c_int * len(lens))(*lens)
            p = lambda a: a.ctypes.data_as(fp)  # noqa: E731
            L.nr_run(n, mu, p(init), p(src), p(ref), len(lens), lens_a, p(y), p(e), p(cf), p(win), p(ex))
            out.update({name + "/num_taps": np.int32(n), name + "/mu": np.float32(mu), name + "/lens": np.asarray(lens, np.int32),
                        name + "/coeffs_init": init, name + "/src": src, name + "/ref": ref, name + "/y": y, name + "/e": e,
                        name + "/coeffs": cf, name + "/window": win, name + "/energy": ex[0:1].copy(), name + "/x0": ex[1:2].copy()})
    out["cases"] = np.array([c[0] for c in CASES])
    out["seed"] = np.int64(SEED)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
