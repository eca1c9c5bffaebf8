"""Writes tests/golden/txcw.npz: the keyed CW path of the TX chain (include/selenite_tx_cw.h, DESIGN.md section 2 "TX CW keyed") composed of
the reference's CMSIS-DSP 1.5.3 functions -- arm_fir_f32 for the keying shape, arm_scale_f32 for the amplitude, arm_fir_interpolate_f32,
arm_cos_f32 / arm_sin_f32 / arm_scale_f32 for the output sample, arm_sin_f32 / arm_scale_f32 / arm_mult_f32 for the sidetone, arm_add_f32
and arm_add_q15 for the speaker mix, arm_float_to_q15 (the truncating build and the ARM_MATH_ROUNDING build) for the int16 forms -- for the
numpy restatement in tests/txcw_oracle.py (tests/test_txcw_oracle.py checks it bit for bit against this file) and for the kernel itself
(tests/test_gpu_txcw.py builds an instance from each stream's parameters).

One channel per stream, at most 512 outputs, filters from zero state, seeded.  Per stream: the key bytes, the shape and interpolator
taps, {amplitude, side_level}, {block, L, step_eff, phase0, side_step, side_phase0, nco_step, offset_step, cwr}:
  dits      a dit string with single-sample dits among it, 16-tap Hann shape, L = 4, P = 8, CW, NCO on; key bytes other than 0 and 1
  hard      ns = 1 (hard keying), L = 1, CWR without NCO (zero-IF at -pitch), amplitude 0.5, a random key
  long      97 unsymmetric taps of both signs (the order of the taps shows) over blocks of 32, L = 2, P = 4, amplitude -0.7, both phases
            start at 0xFFFFFF00 and wrap, a sidetone level that saturates the int16 forms
  held      the key down from the first sample to the last, 64-tap Hann shape, L = 4, P = 16 (the steady state of the shape)
Kept per stream: e, a, u, out (f32), both int16 builds of out, the sidetone y, its f32 mix into `side_in`, both int16 builds of y and of
its saturating mix into `side_in_q15` (which holds +-32767, +-32768 and ordinary values), the phases behind the last sample.
`addq15/a`, `addq15/b`, `addq15/sum`: arm_add_q15 alone on pairs that saturate at both ends and pairs that do not.

The reference files and the small harness below are compiled into a temporary directory with oracle/Makefile's flags (-std=gnu11 -O2
-ffp-contract=off -DARM_MATH_CM4), run, and deleted (arm_add_q15.c's Cortex-M4 path is built on the QADD16 instruction, which the harness
states in C): nothing compiled is kept, and no test or build step compiles reference code.  Run by
hand where the reference tree is:
    python3 tests/golden/make_txcw_golden.py REFERENCE_ROOT      (the root of the reference firmware tree)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "txcw.npz")

HARNESS = r"""
#include <stdlib.h>
#include "arm_math.h"
/* arm_add_q15.c's Cortex-M4 path adds two q15 pairs per QADD16 instruction; off the target the instruction has no definition, so it is
 * stated here as the architecture manual does: each half-word sum saturated to 16 bits */
uint32_t __QADD16(uint32_t x, uint32_t y)
{
    int32_t lo = (int32_t)(int16_t)(x & 0xFFFFu) + (int32_t)(int16_t)(y & 0xFFFFu), hi = (int32_t)(int16_t)(x >> 16) + (int32_t)(int16_t)(y >> 16);
    lo = lo > 32767 ? 32767 : (lo < -32768 ? -32768 : lo);
    hi = hi > 32767 ? 32767 : (hi < -32768 ? -32768 : hi);
    return ((uint32_t)hi << 16) | ((uint32_t)lo & 0xFFFFu);
}
/* one stream, DSP block by DSP block as DESIGN.md section 2 writes the keyed path; par = {amplitude, side_level},
 * ipar = {block, L, step_eff, phase0, side_step, side_phase0}; phases_out = {nco_phase, side_phase} behind the last sample */
int txcw_run(int N, const uint8_t *key, int ns, const float *shape, int ni, const float *ic, const float *par, const uint32_t *ipar,
             float *e, float *a, float *u, float *out, int16_t *q15, float *y, int16_t *yq, const float *side_in, float *side_mix,
             const int16_t *side_in_q, int16_t *side_mix_q, uint32_t *phases_out)
{
    const uint32_t nb = ipar[0], L = ipar[1];
    uint32_t phase = ipar[3], sp = ipar[5];
    arm_fir_instance_f32 F;
    arm_fir_interpolate_instance_f32 I;
    float *fs = calloc(ns + nb - 1, sizeof(float)), *is = calloc((ni ? ni / L : 1) + nb - 1, sizeof(float)), *e0 = malloc(nb * sizeof(float));
    arm_fir_init_f32(&F, ns, (float *)shape, fs, nb);
    if (ni && arm_fir_interpolate_init_f32(&I, L, ni, (float *)ic, is, nb) != ARM_MATH_SUCCESS) return 1;
    for (int b = 0; b < N / (int)nb; ++b) {
        const int at = b * nb;
        for (uint32_t i = 0; i < nb; ++i) e0[i] = key[at + i] ? 1.0f : 0.0f;
        arm_fir_f32(&F, e0, e + at, nb);
        arm_scale_f32(e + at, par[0], a + at, nb);
        if (ni) arm_fir_interpolate_f32(&I, a + at, u + at * L, nb);
        else for (uint32_t i = 0; i < nb; ++i) u[at + i] = a[at + i];
        for (uint32_t m = at * L; m < (at + nb) * L; ++m) {
            float x = (float)(phase >> 8) * 0x1.921fb6p-22f, c = arm_cos_f32(x), s = arm_sin_f32(x);
            arm_scale_f32(&c, u[m], out + 2 * m, 1);
            arm_scale_f32(&s, u[m], out + 2 * m + 1, 1);
            phase += ipar[2];
        }
        for (uint32_t n = at; n < at + nb; ++n) {
            float xs = (float)(sp >> 8) * 0x1.921fb6p-22f, s = arm_sin_f32(xs), g;
            arm_scale_f32(e + n, par[1], &g, 1);
            arm_mult_f32(&s, &g, y + n, 1);
            sp += ipar[4];
        }
    }
    arm_float_to_q15(out, q15, 2u * (uint32_t)N * L);
    arm_float_to_q15(y, yq, (uint32_t)N);
    arm_add_f32((float *)side_in, y, side_mix, (uint32_t)N);
    arm_add_q15((q15_t *)side_in_q, yq, side_mix_q, (uint32_t)N);
    phases_out[0] = phase;
    phases_out[1] = sp;
    free(fs); free(is); free(e0);
    return 0;
}
"""

SEED = 0x54584357
f32 = np.float32


def hann(ns):
    k = np.arange(ns, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * (k + 1) / (ns + 1))
    return (w / w.sum()).astype(f32)


def lowpass(ni, L):
    """a windowed-sinc interpolation low-pass of gain L (any finite taps serve: they are stored in the fixture)"""
    if not ni:
        return np.zeros(0, f32)
    n = np.arange(ni, dtype=np.float64) - (ni - 1) / 2
    h = np.sinc(0.8 * n / L) * np.hamming(ni)
    return (h / h.sum() * L).astype(f32)


def streams():
    rng = np.random.default_rng(SEED)
    S = {}
    k = np.zeros(128, np.uint8)
    for at, n in ((3, 20), (40, 1), (43, 1), (50, 30), (100, 27)):                       # the last element runs into the end of the stream
        k[at:at + n] = 1
    k[5], k[52], k[40] = 0xFF, 2, 0x80
    S["dits"] = dict(key=k, shape=hann(16), block=64, L=4, ni=32, amplitude=0.9, nco_step=0x0A5F1C27, offset_step=0x00DA740E, cwr=0, phase0=0x12345678,
                     side_level=0.25, side_step=0x0DA740DA, side_phase0=0)
    S["hard"] = dict(key=(rng.uniform(size=256) < 0.5).astype(np.uint8), shape=np.ones(1, f32), block=64, L=1, ni=0, amplitude=0.5, nco_step=0,
                     offset_step=0x0DA740DA, cwr=1, phase0=0, side_level=0.999, side_step=0x11111111, side_phase0=0x80000000)
    kl = np.repeat((rng.uniform(size=24) < 0.5).astype(np.uint8), 8)
    kl[60:64] = 1
    S["long"] = dict(key=kl, shape=(rng.uniform(-1, 1, 97) / 20).astype(f32), block=32, L=2, ni=8, amplitude=-0.7, nco_step=0xC0000001,
                     offset_step=0x00400000, cwr=1, phase0=0xFFFFFF00, side_level=30.0, side_step=0x10000101, side_phase0=0xFFFFFF00)
    S["held"] = dict(key=np.ones(128, np.uint8), shape=hann(64), block=64, L=4, ni=64, amplitude=1.0, nco_step=0x01000000, offset_step=0x00DA740E,
                     cwr=0, phase0=0, side_level=0.5, side_step=0x0DA740DA, side_phase0=0x40000000)
    return S, rng


def main(ref_root):
    dsp = os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Source")
    inc = ["-I" + os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Include"), "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Core", "Include"),
           "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Include")]
    names = ["FilteringFunctions/arm_fir_f32.c", "FilteringFunctions/arm_fir_init_f32.c", "FilteringFunctions/arm_fir_interpolate_f32.c",
             "FilteringFunctions/arm_fir_interpolate_init_f32.c", "BasicMathFunctions/arm_scale_f32.c", "BasicMathFunctions/arm_mult_f32.c",
             "BasicMathFunctions/arm_add_f32.c", "BasicMathFunctions/arm_add_q15.c", "FastMathFunctions/arm_sin_f32.c",
             "FastMathFunctions/arm_cos_f32.c", "CommonTables/arm_common_tables.c"]
    srcs = [os.path.join(dsp, *n.split("/")) for n in names]
    q15 = os.path.join(dsp, "SupportFunctions", "arm_float_to_q15.c")
    flags = ["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-w", "-DARM_MATH_CM4"] + inc
    S, rng = streams()
    out = {"names": np.array(sorted(S))}
    with tempfile.TemporaryDirectory() as tmp:
        h = os.path.join(tmp, "harness.c")
        with open(h, "w") as f:
            f.write(HARNESS)
        so, so_r = os.path.join(tmp, "libtxcw.so"), os.path.join(tmp, "libtxcw_r.so")
        subprocess.run(flags + ["-shared", "-o", so, h, q15] + srcs + ["-lm"], check=True)
        subprocess.run(flags + ["-DARM_MATH_ROUNDING", "-shared", "-o", so_r, h, q15] + srcs + ["-lm"], check=True)   # arm_float_to_q15's other build
        vp = C.c_void_p
        libs = []
        for path in (so, so_r):
            L_ = C.CDLL(path)
            L_.txcw_run.argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, vp] + [vp] * 12
            L_.arm_add_q15.argtypes = [vp, vp, vp, C.c_uint32]
            L_.arm_add_q15.restype = None
            libs.append(L_)
        for name, s in S.items():
            key = np.ascontiguousarray(s["key"], np.uint8)
            N, L, nb = key.size, s["L"], s["block"]
            assert N % nb == 0 and N * L <= 512
            shape, ic = np.ascontiguousarray(s["shape"], f32), lowpass(s["ni"], L)
            assert np.isfinite(shape).all() and np.isfinite(ic).all()
            off = s["offset_step"] if not s["cwr"] else (-s["offset_step"]) & 0xFFFFFFFF
            par = np.array([s["amplitude"], s["side_level"]], f32)
            ipar = np.array([nb, L, (s["nco_step"] + off) & 0xFFFFFFFF, s["phase0"], s["side_step"], s["side_phase0"]], np.uint32)
            side_in = rng.uniform(-0.5, 0.5, N).astype(f32)
            side_in_q = rng.integers(-20000, 20000, N).astype(np.int16)
            side_in_q[0:8] = [32767, -32768, 32767, -32768, -32767, 32767, 0, 1]
            side_in_q[N // 2::4] = 32767
            side_in_q[N // 2 + 1::4] = -32767
            res = {}
            for tag, L_ in zip(("trunc", "round"), libs):
                e, a, y, mix = (np.zeros(N, f32) for _ in range(4))
                u, o = np.zeros(N * L, f32), np.zeros((N * L, 2), f32)
                q, yq, mixq = np.zeros((N * L, 2), np.int16), np.zeros(N, np.int16), np.zeros(N, np.int16)
                ph = np.zeros(2, np.uint32)
                rc_ = L_.txcw_run(N, key.ctypes.data, shape.size, shape.ctypes.data, ic.size, ic.ctypes.data if ic.size else None, par.ctypes.data,
                                  ipar.ctypes.data, e.ctypes.data, a.ctypes.data, u.ctypes.data, o.ctypes.data, q.ctypes.data, y.ctypes.data,
                                  yq.ctypes.data, side_in.ctypes.data, mix.ctypes.data, side_in_q.ctypes.data, mixq.ctypes.data, ph.ctypes.data)
                assert rc_ == 0 and np.isfinite(o).all()
                res[tag] = dict(e=e, a=a, u=u, out=o, y=y, side_mix=mix, phases=ph, q15=q, yq=yq, side_mix_q=mixq)
            for k_ in ("e", "a", "u", "out", "y", "side_mix", "phases"):                  # the f32 path does not depend on the q15 build
                assert res["trunc"][k_].tobytes() == res["round"][k_].tobytes()
                out[name + "/" + k_] = res["trunc"][k_]
            for tag in ("trunc", "round"):
                out[name + "/q15_" + tag] = res[tag]["q15"]
                out[name + "/yq_" + tag] = res[tag]["yq"]
                out[name + "/side_mix_q_" + tag] = res[tag]["side_mix_q"]
            cfg = np.array([nb, L, s["nco_step"], s["offset_step"], s["cwr"], s["phase0"], s["side_step"], s["side_phase0"]], np.uint32)
            for k_, v in dict(key=key, shape=shape, ic=ic, par=par, ipar=ipar, cfg=cfg, side_in=side_in, side_in_q15=side_in_q).items():
                out[name + "/" + k_] = v
        qa = np.array([32767, 32767, -32768, -32768, 20000, -20000, 100, -100, 0, 32767, -32768, 1], np.int16)
        qb = np.array([1, 32767, -1, -32768, 20000, -20000, -300, 300, 0, -32768, 32767, -1], np.int16)
        qs = np.zeros_like(qa)
        libs[0].arm_add_q15(qa.ctypes.data, qb.ctypes.data, qs.ctypes.data, qa.size)
        out["addq15/a"], out["addq15/b"], out["addq15/sum"] = qa, qb, qs
    # what the issue asks the fixture to hold
    assert (qs == 32767).sum() >= 2 and (qs == -32768).sum() >= 2
    assert (np.abs(out["long/side_mix_q_trunc"].astype(int)) >= 32767).any() and (out["long/side_mix_q_trunc"] == -32768).any()
    assert (out["long/side_mix_q_trunc"] == 32767).any()
    assert not np.array_equal(out["dits/q15_trunc"], out["dits/q15_round"])
    assert (out["long/yq_trunc"] == 32767).any() and (out["long/yq_trunc"] == -32768).any()
    assert out["long/phases"][0] < 0xFFFFFF00 and len(set(np.round(out["held/e"][64:], 9))) == 1
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
