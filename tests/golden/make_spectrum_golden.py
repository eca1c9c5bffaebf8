"""Writes tests/golden/spectrum.npz: arm_cmplx_mult_real_f32 -> arm_cfft_f32 (forward, natural order) -> arm_cmplx_mag_squared_f32 of the
reference's CMSIS-DSP 1.5.3 on seeded frames of 64 and 512 points, with and without a window, and its two twiddle tables, for the numpy
restatement in tests/spectrum_oracle.py (tests/test_spectrum_oracle.py checks it bit for bit against this file).

The reference files (TransformFunctions/arm_cfft_f32.c, arm_cfft_radix8_f32.c, CommonTables/arm_common_tables.c,
ComplexMathFunctions/arm_cmplx_mult_real_f32.c, arm_cmplx_mag_squared_f32.c) and the small harness below are compiled into a temporary
directory with oracle/Makefile's flags (-std=gnu11 -O2 -ffp-contract=off -DARM_MATH_CM4), run, and deleted: nothing compiled is kept, and
no test or build step compiles reference code.  Run by hand where the reference tree is:
    python3 tests/golden/make_spectrum_golden.py REFERENCE_ROOT      (the root of the reference firmware tree)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "spectrum.npz")

# our harness.  The instance is built here from twiddleCoef_N / armBitRevIndexTableN (arm_const_structs.c drags in unrelated q15 tables),
# and arm_bitreversal_32, which the reference has only as Thumb assembly (arm_bitreversal2.S), is its C meaning: the table holds pairs of
# byte offsets into the float array; the two 8-byte elements of a pair are swapped.
HARNESS = r"""
#include "arm_math.h"
#include "arm_common_tables.h"
#include <string.h>
void arm_bitreversal_32(uint32_t *pSrc, const uint16_t bitRevLen, const uint16_t *pBitRevTab)
{
    for (uint32_t i = 0; i + 1 < bitRevLen; i += 2) {
        const uint32_t a = pBitRevTab[i] >> 2, b = pBitRevTab[i + 1] >> 2;
        uint32_t t = pSrc[a]; pSrc[a] = pSrc[b]; pSrc[b] = t;
        t = pSrc[a + 1]; pSrc[a + 1] = pSrc[b + 1]; pSrc[b + 1] = t;
    }
}
int spec_run(int n, int nframes, const float *frames, const float *window, float *fft, float *power)
{
    arm_cfft_instance_f32 S;
    if (n == 64) { S.fftLen = 64; S.pTwiddle = twiddleCoef_64; S.pBitRevTable = armBitRevIndexTable64; S.bitRevLength = ARMBITREVINDEXTABLE_64_TABLE_LENGTH; }
    else if (n == 512) { S.fftLen = 512; S.pTwiddle = twiddleCoef_512; S.pBitRevTable = armBitRevIndexTable512; S.bitRevLength = ARMBITREVINDEXTABLE_512_TABLE_LENGTH; }
    else return -1;
    for (int f = 0; f < nframes; ++f) {
        float *p = fft + (size_t)f * 2 * n;
        memcpy(p, frames + (size_t)f * 2 * n, sizeof(float) * 2 * n);
        if (window) arm_cmplx_mult_real_f32(p, (float32_t *)window, p, (uint32_t)n);
        arm_cfft_f32(&S, p, 0, 1);
        arm_cmplx_mag_squared_f32(p, power + (size_t)f * n, (uint32_t)n);
    }
    return 0;
}
void spec_tables(float *t64, float *t512)
{
    memcpy(t64, twiddleCoef_64, sizeof(float) * 128);
    memcpy(t512, twiddleCoef_512, sizeof(float) * 1024);
}
"""

SEED = 0x53504543
# the frames of either length, in this order (NAMES is stored); the frame with the Inf sample is the last one
NAMES = ["tone_bin5", "tone_bin_minus3", "tone_between_bins", "two_tones_noise_-80dB", "noise_-40dB", "noise_full_scale", "silent",
         "minus_zero", "level_1e-22", "level_1e18", "int16_slot_values", "noise_-20dB_dc", "inf_sample"]


def frames_of(n, rng):
    t = np.arange(n)
    noise = lambda lvl: lvl * (rng.uniform(-1, 1, (n, 2)))  # noqa: E731
    tone = lambda k, a=0.5, ph=0.3: a * np.stack([np.cos(2 * np.pi * k * t / n + ph), np.sin(2 * np.pi * k * t / n + ph)], axis=1)  # noqa: E731
    fr = [tone(5), tone(n - 3), tone(7.5), tone(9, 0.4) + tone(n // 2 + 3.25, 0.05) + noise(1e-4), noise(1e-2), noise(1.0),
          np.zeros((n, 2))]
    mz = np.full((n, 2), -0.0)
    mz[::3, 0] = 0.0
    fr += [mz, noise(1e-22), noise(1e18), np.trunc(noise(1.0) * 32768.0) / 32768.0, noise(0.1) + 0.25]
    inf = noise(0.5)
    inf[n // 3, 1] = np.inf
    fr.append(inf)
    return np.ascontiguousarray(np.stack(fr), np.float32)


def main(ref_root):
    dsp = os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Source")
    inc = ["-I" + os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Include"), "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Core", "Include"),
           "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Include")]
    srcs = [os.path.join(dsp, "TransformFunctions", "arm_cfft_f32.c"), os.path.join(dsp, "TransformFunctions", "arm_cfft_radix8_f32.c"),
            os.path.join(dsp, "CommonTables", "arm_common_tables.c"), os.path.join(dsp, "ComplexMathFunctions", "arm_cmplx_mult_real_f32.c"),
            os.path.join(dsp, "ComplexMathFunctions", "arm_cmplx_mag_squared_f32.c")]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        h = os.path.join(tmp, "harness.c")
        with open(h, "w") as f:
            f.write(HARNESS)
        so = os.path.join(tmp, "libspec.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-w", "-DARM_MATH_CM4"] + inc + ["-shared", "-o", so, h] + srcs,
                       check=True)
        L = C.CDLL(so)
        fp = C.POINTER(C.c_float)
        L.spec_run.argtypes = [C.c_int, C.c_int, fp, fp, fp, fp]
        L.spec_tables.argtypes = [fp, fp]
        p = lambda a: a.ctypes.data_as(fp)  # noqa: E731
        t64, t512 = np.empty((64, 2), np.float32), np.empty((512, 2), np.float32)
        L.spec_tables(p(t64), p(t512))
        out["twiddle64"], out["twiddle512"] = t64, t512
        rng = np.random.default_rng(SEED)
        for n in (64, 512):
            fr = frames_of(n, rng)
            # a Hann window with a little of everything on top (no structure a symmetric window would hide), and an exact zero
            win = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n) + 0.01 * rng.standard_normal(n)).astype(np.float32)
            win[0] = 0.0
            out["n%d/frames" % n], out["n%d/window" % n] = fr, win
            for tag, w in (("plain", None), ("windowed", win)):
                fft, pw = np.empty_like(fr), np.empty(fr.shape[:2], np.float32)
                assert L.spec_run(n, fr.shape[0], p(fr), p(w) if w is not None else None, p(fft), p(pw)) == 0
                out["n%d/%s/fft" % (n, tag)], out["n%d/%s/power" % (n, tag)] = fft, pw
    out["names"] = np.array(NAMES)
    out["seed"] = np.int64(SEED)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
