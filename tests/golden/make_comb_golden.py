"""Writes tests/golden/comb.npz: the polyphase combiner's composition (include/selenite_comb.h) -- per input frame arm_cfft_f32 (inverse,
natural order), per output sample and rail arm_dot_prod_f32 over the Q = P * oversample frames that overlap in it, and arm_float_to_q15 in
both of its builds for the int16 output -- run with the reference's CMSIS-DSP 1.5.3 functions on seeded channel rows, for the numpy
restatement in tests/comb_oracle.py (tests/test_comb_oracle.py checks it bit for bit against this file, outputs and history).

The reference files (BasicMathFunctions/arm_dot_prod_f32.c, TransformFunctions/arm_cfft_f32.c, arm_cfft_radix8_f32.c,
CommonTables/arm_common_tables.c, SupportFunctions/arm_float_to_q15.c twice: as the firmware builds it and with -DARM_MATH_ROUNDING) and the
small harness below are compiled into a temporary directory with oracle/Makefile's flags (-std=gnu11 -O2 -ffp-contract=off -DARM_MATH_CM4),
run, and deleted: nothing compiled is kept, and no test or build step compiles reference code.  Run by hand where the reference tree is:
    python3 tests/golden/make_comb_golden.py REFERENCE_ROOT      (the root of the reference firmware tree)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "comb.npz")

# our harness.  The cfft instance and arm_bitreversal_32 as in make_chan_golden.py.  v_in holds one frame of K bins per input frame, the bins
# nobody feeds +0.0f; the transforms of the Q newest frames are kept, frames in front of the stream are +0.0f.
HARNESS = r"""
#include "arm_math.h"
#include "arm_common_tables.h"
#include <string.h>
void arm_float_to_q15_rounding(float32_t *pSrc, q15_t *pDst, uint32_t blockSize);
void arm_bitreversal_32(uint32_t *pSrc, const uint16_t bitRevLen, const uint16_t *pBitRevTab)
{
    for (uint32_t i = 0; i + 1 < bitRevLen; i += 2) {
        const uint32_t a = pBitRevTab[i] >> 2, b = pBitRevTab[i + 1] >> 2;
        uint32_t t = pSrc[a]; pSrc[a] = pSrc[b]; pSrc[b] = t;
        t = pSrc[a + 1]; pSrc[a + 1] = pSrc[b + 1]; pSrc[b + 1] = t;
    }
}
int comb_run(int k, int q, int d, int nframes, const float *v_in, const float *g, float *out)
{
    arm_cfft_instance_f32 S;
    static float32_t u[16][1024];
    float32_t a[16], si[16], sq[16];
    if (k == 64) { S.fftLen = 64; S.pTwiddle = twiddleCoef_64; S.pBitRevTable = armBitRevIndexTable64; S.bitRevLength = ARMBITREVINDEXTABLE_64_TABLE_LENGTH; }
    else if (k == 512) { S.fftLen = 512; S.pTwiddle = twiddleCoef_512; S.pBitRevTable = armBitRevIndexTable512; S.bitRevLength = ARMBITREVINDEXTABLE_512_TABLE_LENGTH; }
    else return -1;
    if (q > 16) return -1;
    for (int f = 0; f < nframes; ++f) {
        float32_t *uf = u[f % q];
        memcpy(uf, v_in + (size_t)f * 2 * k, sizeof(float) * 2 * k);
        arm_cfft_f32(&S, uf, 1, 1);
        for (int j = 0; j < d; ++j) {
            const size_t n = (size_t)f * d + j;
            const int p = (int)(n % (size_t)k);
            for (int t = 0; t < q; ++t) {
                const int fr = f - q + 1 + t;
                a[t] = g[(d - 1 - j) + t * d];
                si[t] = fr < 0 ? 0.0f : u[fr % q][2 * p];
                sq[t] = fr < 0 ? 0.0f : u[fr % q][2 * p + 1];
            }
            arm_dot_prod_f32(a, si, (uint32_t)q, &out[2 * n]);
            arm_dot_prod_f32(a, sq, (uint32_t)q, &out[2 * n + 1]);
        }
    }
    return 0;
}
void comb_q15(float *src, short *dst, unsigned n, int rounding)
{
    if (rounding) arm_float_to_q15_rounding(src, dst, n);
    else arm_float_to_q15(src, dst, n);
}
"""

SEED = 0x434F4D42
# (K, P, oversample, frames, frames of the first of the two calls, rows per band: 0 = all bins)
CASES = [(64, 4, 1, 40, 13, 0), (64, 8, 2, 40, 11, 0), (512, 4, 2, 16, 5, 64)]
Q15_CASE = "k64_p8_o2"


def prototype(k, p, ovs, width):
    """the design of selenite_comb_design_prototype (a Hamming-windowed sinc of unity DC gain times K * D, CMSIS order)"""
    n = k * p
    m = np.arange(n) - (n - 1) / 2.0
    h = np.sinc(width / k * m) * (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n) / (n - 1)))
    return h[::-1] / h.sum() * k * (k // ovs)


def rows_of(nrows, frames, rng):
    """per row a slow tone at 0.5 over noise at -60 dB; full-scale noise; noise at 1e-22 (denormal products); -0.0f with a few +0.0f"""
    t = np.arange(frames)
    f = rng.uniform(-0.05, 0.05, nrows)[:, None]
    ph = rng.uniform(0, 2 * np.pi, nrows)[:, None]
    x = 0.5 * np.stack([np.cos(2 * np.pi * f * t + ph), np.sin(2 * np.pi * f * t + ph)], axis=2) + 1e-3 * rng.uniform(-1, 1, (nrows, frames, 2))
    q = frames // 4
    x[:, q:2 * q] = rng.uniform(-1, 1, (nrows, q, 2))
    x[::2, q, 0], x[1::2, q + 1, 1] = 1.0, -1.0
    x[:, 2 * q:3 * q] = 1e-22 * rng.uniform(-1, 1, (nrows, q, 2))
    x[:, 3 * q:] = -0.0
    x[::3, 3 * q::2, 0] = 0.0
    return np.ascontiguousarray(x, np.float32)


def main(ref_root):
    dsp = os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Source")
    inc = ["-I" + os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Include"), "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Core", "Include"),
           "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Include")]
    srcs = [os.path.join(dsp, "BasicMathFunctions", "arm_dot_prod_f32.c"), os.path.join(dsp, "TransformFunctions", "arm_cfft_f32.c"),
            os.path.join(dsp, "TransformFunctions", "arm_cfft_radix8_f32.c"), os.path.join(dsp, "CommonTables", "arm_common_tables.c"),
            os.path.join(dsp, "SupportFunctions", "arm_float_to_q15.c")]
    flags = ["-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-w", "-DARM_MATH_CM4"]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        h = os.path.join(tmp, "harness.c")
        with open(h, "w") as f:
            f.write(HARNESS)
        ro = os.path.join(tmp, "q15_rounding.o")
        subprocess.run(["gcc"] + flags + ["-DARM_MATH_ROUNDING", "-Darm_float_to_q15=arm_float_to_q15_rounding"] + inc + ["-c", "-o", ro, srcs[-1]],
                       check=True)
        so = os.path.join(tmp, "libcomb.so")
        subprocess.run(["gcc"] + flags + inc + ["-shared", "-o", so, h, ro] + srcs, check=True)
        L = C.CDLL(so)
        fp, sp = C.POINTER(C.c_float), C.POINTER(C.c_short)
        L.comb_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, fp]
        L.comb_q15.argtypes = [fp, sp, C.c_uint, C.c_int]
        L.comb_q15.restype = None
        p_ = lambda a: a.ctypes.data_as(fp)  # noqa: E731
        rng = np.random.default_rng(SEED)

        def run(k, q, d, g, x, bins):
            frames = x.shape[1]
            v = np.zeros((frames, k, 2), np.float32)
            v[:, bins] = np.transpose(x, (1, 0, 2))
            y = np.empty((frames * d, 2), np.float32)
            assert L.comb_run(k, q, d, frames, p_(v), p_(g), p_(y)) == 0
            return y

        names = []
        for k, p, ovs, frames, cut, nrows in CASES:
            d, q = k // ovs, p * ovs
            tag = "k%d_p%d_o%d" % (k, p, ovs)
            g = (prototype(k, p, ovs, 1.0) * (1.0 + 0.01 * rng.standard_normal(k * p))).astype(np.float32)
            if nrows:
                bins = np.concatenate([[0, 255, 256, 511], rng.permutation(np.setdiff1d(np.arange(k), [0, 255, 256, 511]))[:nrows - 4]])
                bins = rng.permutation(bins).astype(np.int64)
            else:
                bins = np.arange(k)
            x = rows_of(len(bins), frames, rng)
            y = run(k, q, d, g, x, bins)
            out[tag + "/coeffs"], out[tag + "/rows"], out[tag + "/bins"] = g, x, bins.astype(np.uint32)
            out[tag + "/out"] = y                                                        # [frames * D][2]: the object's layout for one band
            out[tag + "/history"] = x[:, frames - (q - 1):]                              # what the state holds behind the stream
            out[tag + "/cut"] = np.int64(cut)
            if tag == Q15_CASE:
                xs = (x * np.float32(0.25)).astype(np.float32)
                ys = run(k, q, d, g, xs, bins)
                out[tag + "/q15_rows"] = xs
                for r, name in ((0, "trunc"), (1, "round")):
                    z = np.empty(ys.shape, np.int16)
                    L.comb_q15(p_(ys), z.ctypes.data_as(sp), ys.size, r)
                    sat = int((np.abs(z.astype(np.int32)) >= 32767).sum())
                    assert 0 < sat < z.size // 4, sat                                    # some samples saturate, most do not
                    assert (z == 32767).any() and (z == -32768).any()
                    out[tag + "/q15_" + name] = z
                assert (out[tag + "/q15_trunc"] != out[tag + "/q15_round"]).any()
            names.append(tag)
    out["names"] = np.array(names)
    out["seed"] = np.int64(SEED)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
