"""Writes tests/golden/chan.npz: the polyphase channeliser's composition (include/selenite_chan.h) -- per output and FFT position
arm_dot_prod_f32 over the P samples K apart, per rail, the rotation by n0, then arm_cfft_f32 (forward, natural order) -- run with the
reference's CMSIS-DSP 1.5.3 functions on seeded streams, for the numpy restatement in tests/chan_oracle.py (tests/test_chan_oracle.py
checks it bit for bit against this file, outputs and history).

The reference files (BasicMathFunctions/arm_dot_prod_f32.c, TransformFunctions/arm_cfft_f32.c, arm_cfft_radix8_f32.c,
CommonTables/arm_common_tables.c) and the small harness below are compiled into a temporary directory with oracle/Makefile's flags
(-std=gnu11 -O2 -ffp-contract=off -DARM_MATH_CM4), run, and deleted: nothing compiled is kept, and no test or build step compiles reference
code.  Run by hand where the reference tree is:
    python3 tests/golden/make_chan_golden.py REFERENCE_ROOT      (the root of the reference firmware tree)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "chan.npz")

# our harness.  The cfft instance and arm_bitreversal_32 as in make_spectrum_golden.py (the reference has the latter only as Thumb assembly:
# the table holds pairs of byte offsets into the float array; the two 8-byte elements of a pair are swapped).  The stream is handed over with
# its K P - D samples of history in front, so the window of output m starts at sample m D.
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
int chan_run(int k, int p, int d, int nout, unsigned long long position, const float *stream, const float *g, float *out)
{
    arm_cfft_instance_f32 S;
    float32_t a[16], si[16], sq[16], v[1024];
    if (k == 64) { S.fftLen = 64; S.pTwiddle = twiddleCoef_64; S.pBitRevTable = armBitRevIndexTable64; S.bitRevLength = ARMBITREVINDEXTABLE_64_TABLE_LENGTH; }
    else if (k == 512) { S.fftLen = 512; S.pTwiddle = twiddleCoef_512; S.pBitRevTable = armBitRevIndexTable512; S.bitRevLength = ARMBITREVINDEXTABLE_512_TABLE_LENGTH; }
    else return -1;
    if (p > 16) return -1;
    for (int m = 0; m < nout; ++m) {
        const float *s = stream + 2 * (size_t)m * d;
        const int n0 = (int)((position + (unsigned long long)(m + 1) * d) % (unsigned long long)k);
        for (int r = 0; r < k; ++r) {
            for (int t = 0; t < p; ++t) { a[t] = g[r + t * k]; si[t] = s[2 * (r + t * k)]; sq[t] = s[2 * (r + t * k) + 1]; }
            arm_dot_prod_f32(a, si, (uint32_t)p, &v[2 * ((r + n0) % k)]);
            arm_dot_prod_f32(a, sq, (uint32_t)p, &v[2 * ((r + n0) % k) + 1]);
        }
        arm_cfft_f32(&S, v, 0, 1);
        memcpy(out + (size_t)m * 2 * k, v, sizeof(float) * 2 * k);
    }
    return 0;
}
"""

SEED = 0x4348414E
# (K, P, oversample, outputs, outputs of the first of the two calls)
CASES = [(64, 4, 1, 32, 13), (64, 4, 2, 32, 11), (512, 4, 2, 14, 5)]


def prototype(k, p, width):
    """the design of selenite_chan_design_prototype (a Hamming-windowed sinc, unity DC gain, CMSIS order), with a little of everything on top so
    that no symmetry of the taps hides an index error"""
    n = k * p
    m = np.arange(n) - (n - 1) / 2.0
    h = np.sinc(width / k * m) * (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n) / (n - 1)))
    return h[::-1] / h.sum()


def stream_of(k, d, nout, rng):
    """tone on bin 5 at 0.5 over noise at -60 dB; full-scale noise; noise at 1e-22 (denormal products); -0.0f with a few +0.0f"""
    L = nout * d
    t = np.arange(L)
    x = 0.5 * np.stack([np.cos(2 * np.pi * 5 * t / k + 0.3), np.sin(2 * np.pi * 5 * t / k + 0.3)], axis=1) + 1e-3 * rng.uniform(-1, 1, (L, 2))
    q = L // 4
    x[q:2 * q] = rng.uniform(-1, 1, (q, 2))
    x[q, 0], x[q + 1, 1] = 1.0, -1.0
    x[2 * q:3 * q] = 1e-22 * rng.uniform(-1, 1, (q, 2))
    x[3 * q:] = -0.0
    x[3 * q::5, 0] = 0.0
    return np.ascontiguousarray(x, np.float32)


def main(ref_root):
    dsp = os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Source")
    inc = ["-I" + os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Include"), "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Core", "Include"),
           "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Include")]
    srcs = [os.path.join(dsp, "BasicMathFunctions", "arm_dot_prod_f32.c"), os.path.join(dsp, "TransformFunctions", "arm_cfft_f32.c"),
            os.path.join(dsp, "TransformFunctions", "arm_cfft_radix8_f32.c"), os.path.join(dsp, "CommonTables", "arm_common_tables.c")]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        h = os.path.join(tmp, "harness.c")
        with open(h, "w") as f:
            f.write(HARNESS)
        so = os.path.join(tmp, "libchan.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-w", "-DARM_MATH_CM4"] + inc + ["-shared", "-o", so, h] + srcs,
                       check=True)
        L = C.CDLL(so)
        fp = C.POINTER(C.c_float)
        L.chan_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, fp, fp, fp]
        p_ = lambda a: a.ctypes.data_as(fp)  # noqa: E731
        rng = np.random.default_rng(SEED)
        names = []
        for k, p, ovs, nout, cut in CASES:
            d = k // ovs
            tag = "k%d_p%d_o%d" % (k, p, ovs)
            g = (prototype(k, p, 1.0 * ovs) * (1.0 + 0.01 * rng.standard_normal(k * p))).astype(np.float32)
            x = stream_of(k, d, nout, rng)
            hist = k * p - d
            full = np.ascontiguousarray(np.concatenate([np.zeros((hist, 2), np.float32), x]))
            y = np.empty((nout, k, 2), np.float32)
            assert L.chan_run(k, p, d, nout, 0, p_(full), p_(g), p_(y)) == 0
            out[tag + "/coeffs"], out[tag + "/stream"] = g, x
            out[tag + "/out"] = np.ascontiguousarray(np.transpose(y, (1, 0, 2)))          # [K][nout][2]: the object's layout for one band
            out[tag + "/history"] = full[len(full) - hist:]                              # what the state holds behind the stream
            out[tag + "/cut"] = np.int64(cut * d)
            names.append(tag)
    out["names"] = np.array(names)
    out["seed"] = np.int64(SEED)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
