"""Writes tests/golden/tones.npz: the tone-detector bank (selenite_rx_set_tones) composed of the reference's CMSIS-DSP 1.5.3 functions --
arm_biquad_cascade_df1_f32 with the one section {1, 0, 0, c, -1} per tone (s1 = y1, s2 = y2), arm_power_f32 for the frame energy,
arm_cmplx_mag_squared_f32 for the powers and arm_max_f32 for the best tone -- for the numpy restatement in tests/tones_oracle.py
(tests/test_tones_oracle.py checks it bit for bit against this file) and for the stage itself (tests/test_gpu_tones.py).

Per case (K tones, frames of N samples) two streams of 2.5 frames, cut into calls of 1, 3, 4, 13, 64 and 200 samples in turn on one running
state, so that calls end frames in their middle:
  0  noise and one tone of the table
  1  noise with +0.0f and denormals in it
All samples are finite and none is -0.0f (on such input the section's dead products 0 * x1, 0 * x2 change no bit).  Kept per call: the
recurrence state of every tone and the running energy behind it; per frame: p[K], E, and arm_max_f32's value and index.

The reference files and the small harness below are compiled into a temporary directory with oracle/Makefile's flags (-std=gnu11 -O2
-ffp-contract=off -DARM_MATH_CM4), run, and deleted: nothing compiled is kept, and no test or build step compiles reference code.  Run by
hand where the reference tree is:
    python3 tests/golden/make_tones_golden.py REFERENCE_ROOT      (the root of the reference firmware tree)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tones_oracle as to  # noqa: E402

OUT = os.path.join(HERE, "tones.npz")

HARNESS = r"""
#include "arm_math.h"
/* one stream: x [T] cut into calls of lens[ncalls] samples, frames of N samples counted from the stream's start.
 * coeffs [K][3] {c, cw, sw}; st [K][4] biquad state {x1, x2, y1, y2}, running, cleared here at a frame's end
 * out: call_s [ncalls][K][2] {s1, s2} and call_e [ncalls] behind every call (e: the energy of the running frame's samples so far);
 *      p [nframes][K], fe, pbest [nframes], best [nframes] */
int tones_run(int K, int N, const float *coeffs, int T, const float *x, int ncalls, const int *lens, float *call_s, float *call_e,
              float *p, float *fe, float *pbest, unsigned *best)
{
    static float st[64][4], k5[64][5], y[4096], ri[128];
    int at = 0, done = 0, frames = 0, f0 = 0;      /* f0: first sample of the running frame */
    for (int k = 0; k < K; ++k) {
        k5[k][0] = 1.0f; k5[k][1] = 0.0f; k5[k][2] = 0.0f; k5[k][3] = coeffs[3 * k]; k5[k][4] = -1.0f;
        st[k][0] = st[k][1] = st[k][2] = st[k][3] = 0.0f;
    }
    for (int c = 0; c < ncalls; ++c) {
        int left = lens[c];
        while (left > 0) {
            int seg = N - done < left ? N - done : left;
            for (int k = 0; k < K; ++k) {
                arm_biquad_casd_df1_inst_f32 S = { 1, st[k], k5[k] };
                arm_biquad_cascade_df1_f32(&S, (float *)x + at, y, (uint32_t)seg);
            }
            at += seg; done += seg; left -= seg;
            if (done == N) {
                for (int k = 0; k < K; ++k) {
                    const float s1 = st[k][2], s2 = st[k][3];
                    const float u = coeffs[3 * k + 1] * s2;
                    ri[2 * k] = s1 - u;
                    ri[2 * k + 1] = coeffs[3 * k + 2] * s2;
                    st[k][0] = st[k][1] = st[k][2] = st[k][3] = 0.0f;
                }
                arm_cmplx_mag_squared_f32(ri, p + (size_t)frames * K, (uint32_t)K);
                arm_power_f32((float *)x + f0, (uint32_t)N, fe + frames);
                uint32_t idx;
                arm_max_f32(p + (size_t)frames * K, (uint32_t)K, pbest + frames, &idx);
                best[frames] = idx;
                ++frames; done = 0; f0 = at;
            }
        }
        for (int k = 0; k < K; ++k) {
            call_s[((size_t)c * K + k) * 2] = st[k][2];
            call_s[((size_t)c * K + k) * 2 + 1] = st[k][3];
        }
        call_e[c] = 0.0f;
        if (done) arm_power_f32((float *)x + f0, (uint32_t)done, call_e + c);
    }
    return frames;
}
"""

SEED = 0x544F4E45
CASES = ((1, 12), (5, 24), (50, 64), (64, 200), (5, 200), (64, 12), (50, 24))      # (K, N): every K and every N of the issue
CUTS = (1, 3, 4, 13, 64, 200)


def calls_of(total):
    lens, at, i = [], 0, 0
    while at < total:
        n = min(CUTS[i % len(CUTS)], total - at)
        lens.append(n)
        at += n
        i += 1
    return np.array(lens, np.int32)


def main(ref_root):
    dsp = os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Source")
    inc = ["-I" + os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Include"), "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Core", "Include"),
           "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Include")]
    srcs = [os.path.join(dsp, "FilteringFunctions", "arm_biquad_cascade_df1_f32.c"), os.path.join(dsp, "StatisticsFunctions", "arm_power_f32.c"),
            os.path.join(dsp, "ComplexMathFunctions", "arm_cmplx_mag_squared_f32.c"), os.path.join(dsp, "StatisticsFunctions", "arm_max_f32.c")]
    out = {"cases": np.array(CASES, np.int64)}
    rng = np.random.default_rng(SEED)
    with tempfile.TemporaryDirectory() as tmp:
        h = os.path.join(tmp, "harness.c")
        with open(h, "w") as f:
            f.write(HARNESS)
        so = os.path.join(tmp, "libtones.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-w", "-DARM_MATH_CM4"] + inc + ["-shared", "-o", so, h] + srcs
                       + ["-lm"], check=True)
        L = C.CDLL(so)
        fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_uint)
        L.tones_run.argtypes = [C.c_int, C.c_int, fp, C.c_int, fp, C.c_int, ip, fp, fp, fp, fp, fp, up]
        for K, N in CASES:
            T = 2 * N + N // 2
            lens = calls_of(T)
            freq = np.sort(rng.uniform(0.004, 0.49, K))
            coeffs = to.design(freq)
            t = np.arange(T)
            x = rng.uniform(-0.3, 0.3, (2, T))
            x[0] += 0.1 * np.cos(2 * np.pi * freq[K // 2] * t + 0.3)
            x = x.astype(np.float32)
            m = max(2, T // 10)
            x[1, rng.choice(T, m, replace=False)] = np.float32(0.0)
            x[1, rng.choice(T, m, replace=False)] = (rng.uniform(-1, 1, m) * 1e-39).astype(np.float32)
            x[1, 0], x[1, 1] = np.float32(0.0), np.float32(1e-42)
            assert np.isfinite(x).all() and not (np.signbit(x) & (x == 0)).any()
            nf = T // N
            cs, ce = np.zeros((2, len(lens), K, 2), np.float32), np.zeros((2, len(lens)), np.float32)
            p, fe, pb, best = np.zeros((2, nf, K), np.float32), np.zeros((2, nf), np.float32), np.zeros((2, nf), np.float32), np.zeros((2, nf), np.uint32)
            for s in range(2):
                got = L.tones_run(K, N, coeffs.ctypes.data_as(fp), T, np.ascontiguousarray(x[s]).ctypes.data_as(fp), len(lens), lens.ctypes.data_as(ip),
                                  cs[s].ctypes.data_as(fp), ce[s].ctypes.data_as(fp), p[s].ctypes.data_as(fp), fe[s].ctypes.data_as(fp),
                                  pb[s].ctypes.data_as(fp), best[s].ctypes.data_as(up))
                assert got == nf
            assert np.isfinite(p).all() and np.isfinite(cs).all()
            key = "k%d_n%d/" % (K, N)
            for k, v in dict(coeffs=coeffs, x=x, lens=lens, call_s=cs, call_e=ce, p=p, fe=fe, pbest=pb, best=best).items():
                out[key + k] = v
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
