"""Writes tests/golden/nb.npz: arm_cmplx_mag_squared_f32 and arm_mean_f32 of the reference's CMSIS-DSP 1.5.3 on seeded frames of 32, 64 and
128 complex samples, and arm_q15_to_float on every int16 value, for the numpy restatement of the noise blanker in tests/nb_oracle.py
(tests/test_nb_oracle.py checks it bit for bit against this file).

The reference files (ComplexMathFunctions/arm_cmplx_mag_squared_f32.c, StatisticsFunctions/arm_mean_f32.c,
SupportFunctions/arm_q15_to_float.c) and the small harness below are compiled into a temporary directory with oracle/Makefile's flags
(-std=gnu11 -O2 -ffp-contract=off -DARM_MATH_CM4), run, and deleted: nothing compiled is kept, and no test or build step compiles reference
code.  Run by hand where the reference tree is:
    python3 tests/golden/make_nb_golden.py REFERENCE_ROOT      (the root of the reference firmware tree)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "nb.npz")

HARNESS = r"""
#include "arm_math.h"
void nb_run(int n, int nframes, const float *frames, float *power, float *mean)
{
    for (int f = 0; f < nframes; ++f) {
        arm_cmplx_mag_squared_f32((float32_t *)frames + (size_t)f * 2 * n, power + (size_t)f * n, (uint32_t)n);
        arm_mean_f32(power + (size_t)f * n, (uint32_t)n, mean + f);
    }
}
void nb_q15(const int16_t *q, float *out, int n) { arm_q15_to_float((q15_t *)q, out, (uint32_t)n); }
"""

SEED = 0x4E424C4B
# the frames of every length, in this order (NAMES is stored); the frames with non-finite samples are the last two
NAMES = ["tone", "noise_-40dB", "noise_full_scale", "noise_with_impulse", "silent", "minus_zero", "level_1e-22", "level_1e18",
         "int16_slot_values", "ascending_magnitudes", "nan_sample", "inf_sample"]


def frames_of(n, rng):
    t = np.arange(n)
    noise = lambda lvl: lvl * rng.uniform(-1, 1, (n, 2))  # noqa: E731
    imp = noise(0.05)
    imp[n // 2] = 4.0
    mz = np.full((n, 2), -0.0)
    mz[::3, 0] = 0.0
    # magnitudes over 2^24: the order of the summation shows in the low bits
    asc = np.stack([2.0 ** (t * 24.0 / n) * (1 + rng.uniform(0, 1, n)), rng.uniform(-1, 1, n)], axis=1)
    fr = [0.5 * np.stack([np.cos(2 * np.pi * 5.3 * t / n), np.sin(2 * np.pi * 5.3 * t / n)], axis=1), noise(1e-2), noise(1.0), imp,
          np.zeros((n, 2)), mz, noise(1e-22), noise(1e18), np.trunc(noise(1.0) * 32768.0) / 32768.0, asc]
    nan, inf = noise(0.5), noise(0.5)
    nan[n // 3, 0] = np.nan
    inf[n // 3, 1] = np.inf
    return np.ascontiguousarray(np.stack(fr + [nan, inf]), np.float32)


def main(ref_root):
    dsp = os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Source")
    inc = ["-I" + os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Include"), "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Core", "Include"),
           "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Include")]
    srcs = [os.path.join(dsp, "ComplexMathFunctions", "arm_cmplx_mag_squared_f32.c"), os.path.join(dsp, "StatisticsFunctions", "arm_mean_f32.c"),
            os.path.join(dsp, "SupportFunctions", "arm_q15_to_float.c")]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        h = os.path.join(tmp, "harness.c")
        with open(h, "w") as f:
            f.write(HARNESS)
        so = os.path.join(tmp, "libnb.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-w", "-DARM_MATH_CM4"] + inc + ["-shared", "-o", so, h] + srcs,
                       check=True)
        L = C.CDLL(so)
        fp = C.POINTER(C.c_float)
        L.nb_run.argtypes = [C.c_int, C.c_int, fp, fp, fp]
        L.nb_q15.argtypes = [C.POINTER(C.c_int16), fp, C.c_int]
        p = lambda a: a.ctypes.data_as(fp)  # noqa: E731
        rng = np.random.default_rng(SEED)
        for n in (32, 64, 128):
            fr = frames_of(n, rng)
            pw, mn = np.empty(fr.shape[:2], np.float32), np.empty(fr.shape[0], np.float32)
            L.nb_run(n, fr.shape[0], p(fr), p(pw), p(mn))
            out["f%d/frames" % n], out["f%d/power" % n], out["f%d/mean" % n] = fr, pw, mn
        q = np.arange(-32768, 32768, dtype=np.int16)
        qf = np.empty(q.size, np.float32)
        L.nb_q15(q.ctypes.data_as(C.POINTER(C.c_int16)), p(qf), q.size)
        out["q15_to_float"] = qf
    out["names"] = np.array(NAMES)
    out["seed"] = np.int64(SEED)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
