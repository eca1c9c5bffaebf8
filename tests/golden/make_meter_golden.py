"""Writes tests/golden/meter.npz: arm_power_f32 of the reference's CMSIS-DSP 1.5.3 and a C division by (float)n, on seeded blocks of
n = 1, 3, 24, 64 and 128 samples, for the numpy restatement of the level meter in tests/meter_oracle.py (tests/test_meter_oracle.py checks
it bit for bit against this file).

The reference file (StatisticsFunctions/arm_power_f32.c) and the small harness below are compiled into a temporary directory with
oracle/Makefile's flags (-std=gnu11 -O2 -ffp-contract=off -DARM_MATH_CM4), run, and deleted: nothing compiled is kept, and no test or build
step compiles reference code.  Run by hand where the reference tree is:
    python3 tests/golden/make_meter_golden.py REFERENCE_ROOT      (the root of the reference firmware tree)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "meter.npz")

HARNESS = r"""
#include "arm_math.h"
/* blocks [nblocks][n]; pw, ms [nblocks] */
void meter_run(int n, int nblocks, const float *blocks, float *pw, float *ms)
{
    for (int b = 0; b < nblocks; ++b) {
        arm_power_f32((float *)blocks + (size_t)b * n, (uint32_t)n, pw + b);
        ms[b] = pw[b] / (float)n;
    }
}
"""

SEED = 0x4D455452     # (the first seed from here at which the ascending block shows the summation order at n = 24, 64 and 128: main() looks for it and stores it)
LENGTHS = (1, 3, 24, 64, 128)
# the blocks of every length, in this order (NAMES is stored); the blocks with a non-finite sample are the last two
NAMES = ["noise_-40dB", "noise_full_scale", "full_scale_square", "silent", "level_1e-22", "int16_slot_values", "ascending_magnitudes",
         "descending_magnitudes", "nan_sample", "inf_sample"]


def blocks_of(n, rng):
    t = np.arange(n)
    noise = lambda lvl: lvl * rng.uniform(-1, 1, n)  # noqa: E731
    # magnitudes over 2^12 (their squares over 2^24): the order of the summation shows in the low bits of the power
    asc = 2.0 ** (t * 12.0 / max(n, 2)) * (1 + rng.uniform(0, 1, n))
    bl = [noise(1e-2), noise(1.0), np.where(t % 2 == 0, 1.0, -1.0), np.zeros(n), noise(1e-22), np.trunc(noise(1.0) * 32768.0) / 32768.0, asc,
          asc[::-1].copy()]
    nan, inf = noise(0.5), noise(0.5)
    nan[n // 3] = np.nan
    inf[n // 3] = np.inf
    return np.ascontiguousarray(np.stack(bl + [nan, inf]), np.float32)


def pairwise(v):
    """another order of the same sum: halves, recursively"""
    if len(v) == 1:
        return v[0]
    return np.float32(pairwise(v[:len(v) // 2]) + pairwise(v[len(v) // 2:]))


def main(ref_root):
    dsp = os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Source")
    inc = ["-I" + os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Include"), "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Core", "Include"),
           "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Include")]
    srcs = [os.path.join(dsp, "StatisticsFunctions", "arm_power_f32.c")]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        h = os.path.join(tmp, "harness.c")
        with open(h, "w") as f:
            f.write(HARNESS)
        so = os.path.join(tmp, "libmeter.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-w", "-DARM_MATH_CM4"] + inc + ["-shared", "-o", so, h] + srcs
                       + ["-lm"], check=True)
        L = C.CDLL(so)
        fp = C.POINTER(C.c_float)
        L.meter_run.argtypes = [C.c_int, C.c_int, fp, fp, fp]
        p = lambda a: a.ctypes.data_as(fp)  # noqa: E731
        for seed in range(SEED, SEED + 64):
            rng, shows = np.random.default_rng(seed), True
            for n in LENGTHS:
                bl = blocks_of(n, rng)
                nb = bl.shape[0]
                pw, ms = np.empty(nb, np.float32), np.empty(nb, np.float32)
                L.meter_run(n, nb, p(bl), p(pw), p(ms))
                # the fixture is there to catch another summation order: summed pairwise, the ascending block must give another power
                if n >= 24:
                    a = bl[NAMES.index("ascending_magnitudes")]
                    shows = shows and pairwise(a * a) != pw[NAMES.index("ascending_magnitudes")]
                for k, v in dict(blocks=bl, pw=pw, ms=ms).items():
                    out["n%d/%s" % (n, k)] = v
            if shows:
                break
        assert shows, "no seed at which a pairwise sum of the ascending block differs at every length"
        for n in LENGTHS[2:]:
            a = out["n%d/blocks" % n][NAMES.index("ascending_magnitudes")]
            assert pairwise(a * a) != out["n%d/pw" % n][NAMES.index("ascending_magnitudes")], n
    out["names"] = np.array(NAMES)
    out["lengths"] = np.array(LENGTHS, np.int64)
    out["seed"] = np.int64(seed)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
