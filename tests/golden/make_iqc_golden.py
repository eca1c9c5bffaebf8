"""Writes tests/golden/iqc.npz: arm_mean_f32, arm_offset_f32, arm_scale_f32, arm_sub_f32, arm_power_f32, arm_dot_prod_f32 and arm_sqrt_f32 of
the reference's CMSIS-DSP 1.5.3 and a C division, composed as the I/Q correction stage composes them, on seeded frames of 32, 64 and 128
complex samples, and arm_q15_to_float on every int16 value, for the numpy restatement of the stage in tests/iqc_oracle.py
(tests/test_iqc_oracle.py checks it bit for bit against this file).

The reference files (StatisticsFunctions/arm_mean_f32.c, arm_power_f32.c, BasicMathFunctions/arm_offset_f32.c, arm_dot_prod_f32.c,
arm_scale_f32.c, arm_sub_f32.c, SupportFunctions/arm_q15_to_float.c; arm_sqrt_f32 is inline in Include/arm_math.h) and the small harness
below are compiled into a temporary directory with oracle/Makefile's flags (-std=gnu11 -O2 -ffp-contract=off -DARM_MATH_CM4), run, and
deleted: nothing compiled is kept, and no test or build step compiles reference code.  Run by hand where the reference tree is:
    python3 tests/golden/make_iqc_golden.py REFERENCE_ROOT      (the root of the reference firmware tree)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "iqc.npz")

HARNESS = r"""
#include "arm_math.h"
/* frames [nframes][n][2]; coef [nframes][4] = dc_i, dc_q, p, g; mean [nframes][2]; rails [nframes][2][n] = i, q; t, u, qout [nframes][n];
 * sums [nframes][3] = pii, pqq, piq; est [nframes][4] = a, r, pii / r, b (b = 0 where arm_sqrt_f32 refuses its argument) */
void iqc_run(int n, int nframes, const float *frames, const float *coef, float *mean, float *rails, float *t, float *u, float *qout,
             float *sums, float *est)
{
    float I[128], Q[128];
    for (int f = 0; f < nframes; ++f) {
        const float *x = frames + (size_t)f * 2 * n, *k = coef + 4 * f;
        float *i = rails + (size_t)f * 2 * n, *q = i + n;
        for (int j = 0; j < n; ++j) { I[j] = x[2 * j]; Q[j] = x[2 * j + 1]; }
        arm_mean_f32(I, (uint32_t)n, mean + 2 * f);
        arm_mean_f32(Q, (uint32_t)n, mean + 2 * f + 1);
        arm_offset_f32(I, -k[0], i, (uint32_t)n);
        arm_offset_f32(Q, -k[1], q, (uint32_t)n);
        arm_scale_f32(i, k[2], t + (size_t)f * n, (uint32_t)n);
        arm_sub_f32(q, t + (size_t)f * n, u + (size_t)f * n, (uint32_t)n);
        arm_scale_f32(u + (size_t)f * n, k[3], qout + (size_t)f * n, (uint32_t)n);
        float *s = sums + 3 * f, *e = est + 4 * f;
        arm_power_f32(i, (uint32_t)n, s);
        arm_power_f32(q, (uint32_t)n, s + 1);
        arm_dot_prod_f32(i, q, (uint32_t)n, s + 2);
        const float a = s[2] / s[0];
        const float ap = a * s[2];
        const float r = s[1] - ap;
        const float d = s[0] / r;
        float b = 0.0f;
        (void)arm_sqrt_f32(d, &b);
        e[0] = a; e[1] = r; e[2] = d; e[3] = b;
    }
}
void iqc_q15(const int16_t *q, float *out, int n) { arm_q15_to_float((q15_t *)q, out, (uint32_t)n); }
"""

SEED = 0x49514332     # (a seed at which the ascending frame shows the summation order at all three lengths: main() checks it)
# the frames of every length, in this order (NAMES is stored); the frames with non-finite samples are the last two
NAMES = ["tone_impaired", "noise_-40dB", "noise_full_scale", "silent", "level_1e-22", "int16_slot_values", "ascending_magnitudes", "q_zero",
         "nan_sample", "inf_sample"]


def frames_of(n, rng):
    t = np.arange(n)
    noise = lambda lvl: lvl * rng.uniform(-1, 1, (n, 2))  # noqa: E731
    w = 2 * np.pi * 5.3 * t / n
    tone = np.stack([0.5 * np.cos(w) - 0.03, 1.08 * 0.5 * np.sin(w + np.deg2rad(4.0)) + 0.02], axis=1)
    # magnitudes over 2^24 on the I rail: the order of the summation shows in the low bits of the mean and of the power
    asc = np.stack([2.0 ** (t * 24.0 / n) * (1 + rng.uniform(0, 1, n)), rng.uniform(-1, 1, n)], axis=1)
    qz = noise(0.3)
    qz[:, 1] = 0.0
    fr = [tone, noise(1e-2), noise(1.0), np.zeros((n, 2)), noise(1e-22), np.trunc(noise(1.0) * 32768.0) / 32768.0, asc, qz]
    nan, inf = noise(0.5), noise(0.5)
    nan[n // 3, 0] = np.nan
    inf[n // 3, 1] = np.inf
    frames = np.ascontiguousarray(np.stack(fr + [nan, inf]), np.float32)
    # dc_i, dc_q, p, g in front of each frame; the frame at 1e-22 keeps dc = 0 so that its products are denormals
    coef = np.stack([rng.uniform(-0.05, 0.05, len(NAMES)), rng.uniform(-0.05, 0.05, len(NAMES)), rng.uniform(-0.2, 0.2, len(NAMES)),
                     rng.uniform(0.8, 1.25, len(NAMES))], axis=1)
    coef[NAMES.index("level_1e-22"), :2] = 0.0
    coef[NAMES.index("q_zero"), 1] = 0.0
    return frames, np.ascontiguousarray(coef, np.float32)


def main(ref_root):
    dsp = os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Source")
    inc = ["-I" + os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Include"), "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Core", "Include"),
           "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Include")]
    srcs = [os.path.join(dsp, "StatisticsFunctions", "arm_mean_f32.c"), os.path.join(dsp, "BasicMathFunctions", "arm_offset_f32.c"),
            os.path.join(dsp, "StatisticsFunctions", "arm_power_f32.c"), os.path.join(dsp, "BasicMathFunctions", "arm_dot_prod_f32.c"),
            os.path.join(dsp, "BasicMathFunctions", "arm_scale_f32.c"), os.path.join(dsp, "BasicMathFunctions", "arm_sub_f32.c"),
            os.path.join(dsp, "SupportFunctions", "arm_q15_to_float.c")]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        h = os.path.join(tmp, "harness.c")
        with open(h, "w") as f:
            f.write(HARNESS)
        so = os.path.join(tmp, "libiqc.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-w", "-DARM_MATH_CM4"] + inc + ["-shared", "-o", so, h] + srcs
                       + ["-lm"], check=True)
        L = C.CDLL(so)
        fp = C.POINTER(C.c_float)
        L.iqc_run.argtypes = [C.c_int, C.c_int] + [fp] * 9
        L.iqc_q15.argtypes = [C.POINTER(C.c_int16), fp, C.c_int]
        p = lambda a: a.ctypes.data_as(fp)  # noqa: E731
        rng = np.random.default_rng(SEED)
        for n in (32, 64, 128):
            fr, coef = frames_of(n, rng)
            nf = fr.shape[0]
            e = lambda *s: np.empty(s, np.float32)  # noqa: E731
            mean, rails, t, u, qout, sums, est = e(nf, 2), e(nf, 2, n), e(nf, n), e(nf, n), e(nf, n), e(nf, 3), e(nf, 4)
            L.iqc_run(n, nf, p(fr), p(coef), p(mean), p(rails), p(t), p(u), p(qout), p(sums), p(est))
            # the fixture is there to catch another summation order: summed backwards, the ascending rail must give another mean and power
            asc, ii = fr[NAMES.index("ascending_magnitudes"), :, 0], rails[NAMES.index("ascending_magnitudes"), 0]
            back, backp = np.float32(0), np.float32(0)
            for v, w in zip(asc[::-1], ii[::-1]):
                back, backp = back + v, backp + w * w
            assert back / np.float32(n) != mean[NAMES.index("ascending_magnitudes"), 0] and backp != sums[NAMES.index("ascending_magnitudes"), 0], n
            for k, v in dict(frames=fr, coef=coef, mean=mean, rails=rails, t=t, u=u, qout=qout, sums=sums, est=est).items():
                out["f%d/%s" % (n, k)] = v
        q = np.arange(-32768, 32768, dtype=np.int16)
        qf = np.empty(q.size, np.float32)
        L.iqc_q15(q.ctypes.data_as(C.POINTER(C.c_int16)), p(qf), q.size)
        out["q15_to_float"] = qf
    out["names"] = np.array(NAMES)
    out["seed"] = np.int64(SEED)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
