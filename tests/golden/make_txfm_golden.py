"""Writes tests/golden/txfm.npz: the FM tail of the TX chain's FM mode (include/selenite_tx_fm.h, DESIGN.md section 2 "TX FM") composed
of the reference's CMSIS-DSP 1.5.3 functions -- arm_sin_f32 / arm_scale_f32 / arm_add_f32 for the tone, arm_scale_f32 and arm_float_to_q31
for the phase increment, arm_cos_f32 / arm_sin_f32 / arm_scale_f32 for the output sample, arm_float_to_q15 (the truncating build and the
ARM_MATH_ROUNDING build) for the int16 output -- for the numpy restatement in tests/txfm_oracle.py (tests/test_txfm_oracle.py checks it
bit for bit against this file) and for the kernel itself (tests/test_gpu_txfm.py: an instance with interp = 1, nh_taps = 0 and the ALC off
takes u as its audio).

Streams of 256 samples `u` (four ALC blocks of 64), seeded; per stream: deviation, amplitude, NCO step, tone on / off with level and step:
  speech     ordinary speech-level values, tone off, a step that wraps the phase every few samples
  speech_t   the same with the tone on, a tone step that wraps tone_phase several times
  zeros      exact +0.0f, -0.0f and denormals among small values, tone off and (zeros_t) tone on
  saturate   v just under and over +1 and -1 (0x7FFFFFFF and 0x80000000 both appear), and far over
  negfrac    v * 2^31 a negative non-integer of a few units: truncation toward zero, not floor
  zero_if    step 0 (nco_enable = 0), amplitude 0.5
  q15, q15_t speech on the q15 grid (u = k / 32768: what the int16 entries hand the chain), tone off / on, phase from 0
All values are finite.  Kept per stream: u, the parameters, d, phase behind every sample, out (f32), both int16 builds of out.

The reference files and the small harness below are compiled into a temporary directory with oracle/Makefile's flags (-std=gnu11 -O2
-ffp-contract=off -DARM_MATH_CM4), run, and deleted: nothing compiled is kept, and no test or build step compiles reference code.  Run by
hand where the reference tree is:
    python3 tests/golden/make_txfm_golden.py REFERENCE_ROOT      (the root of the reference firmware tree)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "txfm.npz")

HARNESS = r"""
#include "arm_math.h"
/* one stream, sample by sample as DESIGN.md section 2 writes the FM tail; par = {deviation, amplitude, tone_level},
 * ipar = {step, phase0, tone_on, tone_step, tone_phase0}; returns the tone phase behind the last sample */
uint32_t txfm_run(int N, const float *u, const float *par, const uint32_t *ipar, int32_t *d_out, uint32_t *phase_out, float *out, int16_t *q15)
{
    uint32_t phase = ipar[1], tp = ipar[4];
    for (int n = 0; n < N; ++n) {
        float w = u[n], v, c, s;
        q31_t d;
        if (ipar[2]) {
            float xt = (float)(tp >> 8) * 0x1.921fb6p-22f, sn = arm_sin_f32(xt), t;
            arm_scale_f32(&sn, par[2], &t, 1);
            arm_add_f32(&w, &t, &w, 1);
            tp += ipar[3];
        }
        arm_scale_f32(&w, par[0], &v, 1);
        arm_float_to_q31(&v, &d, 1);
        phase += (uint32_t)d;
        {
            float x = (float)(phase >> 8) * 0x1.921fb6p-22f;
            c = arm_cos_f32(x);
            s = arm_sin_f32(x);
        }
        arm_scale_f32(&c, par[1], out + 2 * n, 1);
        arm_scale_f32(&s, par[1], out + 2 * n + 1, 1);
        phase += ipar[0];
        d_out[n] = d;
        phase_out[n] = phase;
    }
    arm_float_to_q15(out, q15, 2u * (uint32_t)N);
    return tp;
}
"""

SEED = 0x5458464D
N = 256
f32 = np.float32


def streams():
    rng = np.random.default_rng(SEED)
    t = np.arange(N)
    speech = (0.25 * np.sin(2 * np.pi * 0.013 * t) + 0.1 * np.sin(2 * np.pi * 0.047 * t + 1.0) + rng.uniform(-0.05, 0.05, N)).astype(f32)
    S = {}
    S["speech"] = dict(u=speech, deviation=0.3, amplitude=1.0, step=0x3A5F1C27, phase0=0xF0000000, tone_on=0, tone_level=0.0, tone_step=0, tone_phase0=0)
    S["speech_t"] = dict(u=speech, deviation=0.3, amplitude=0.875, step=0x3A5F1C27, phase0=0x12345678, tone_on=1, tone_level=0.15,
                         tone_step=0x0B4E81B5, tone_phase0=0xFFF00000)
    z = rng.uniform(-1e-3, 1e-3, N).astype(f32)
    z[::4] = f32(0.0)
    z[1::8] = f32(-0.0)
    z[2::8] = (rng.uniform(-1, 1, z[2::8].size) * 1e-39).astype(f32)
    z[3], z[7], z[11] = f32(1e-45), f32(-1e-45), f32(1.1754942e-38)
    S["zeros"] = dict(u=z, deviation=0.5, amplitude=1.0, step=0x80000001, phase0=0, tone_on=0, tone_level=0.0, tone_step=0, tone_phase0=0)
    S["zeros_t"] = dict(u=z, deviation=0.5, amplitude=1.0, step=0x80000001, phase0=7, tone_on=1, tone_level=1e-3, tone_step=0x40000100, tone_phase0=0)
    sat = rng.uniform(-1.0, 1.0, N).astype(f32)
    one = f32(1.0)
    edge = [np.nextafter(one, f32(0)), one, np.nextafter(one, f32(2)), -np.nextafter(one, f32(0)), -one, -np.nextafter(one, f32(2)),
            f32(1.5), f32(-1.5), f32(1000.0), f32(-1000.0), f32(0.99999), f32(-0.99999), f32(3.0e9), f32(-3.0e9)]
    sat[5:5 + len(edge)] = edge
    sat[100:100 + len(edge)] = edge[::-1]
    S["saturate"] = dict(u=sat, deviation=1.0, amplitude=1.0, step=0x01000000, phase0=0, tone_on=0, tone_level=0.0, tone_step=0, tone_phase0=0)
    S["saturate_t"] = dict(u=(sat * f32(0.5)).astype(f32), deviation=2.0, amplitude=1.0, step=0xFEDCBA98, phase0=0x80000000, tone_on=1, tone_level=0.01,
                           tone_step=0xC0000001, tone_phase0=0x00000100)
    k = rng.integers(1, 40, N)
    nf = (-(k + rng.uniform(0.05, 0.95, N)) / 2147483648.0).astype(f32)           # v * 2^31 in (-40, -1), never an integer
    nf[::3] = -nf[::3]                                                             # and their mirror images
    S["negfrac"] = dict(u=nf, deviation=1.0, amplitude=1.0, step=0, phase0=0x00000080, tone_on=0, tone_level=0.0, tone_step=0, tone_phase0=0)
    S["zero_if"] = dict(u=speech[::-1].copy(), deviation=0.45, amplitude=0.5, step=0, phase0=0, tone_on=1, tone_level=0.1, tone_step=0x02345678, tone_phase0=0)
    uq = (np.round(speech.astype(np.float64) * 32768.0) / 32768.0).astype(f32)      # what arm_q15_to_float gives: the int16 entries take int16 audio
    S["q15"] = dict(u=uq, deviation=0.3, amplitude=0.999, step=0x3A5F1C27, phase0=0, tone_on=0, tone_level=0.0, tone_step=0, tone_phase0=0)
    S["q15_t"] = dict(u=uq, deviation=0.3, amplitude=-0.7, step=0xC5A0E3D9, phase0=0, tone_on=1, tone_level=0.15, tone_step=0x0B4E81B5, tone_phase0=0)
    return S


def main(ref_root):
    dsp = os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Source")
    inc = ["-I" + os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Include"), "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Core", "Include"),
           "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Include")]
    srcs = [os.path.join(dsp, "SupportFunctions", "arm_float_to_q31.c"), os.path.join(dsp, "FastMathFunctions", "arm_sin_f32.c"),
            os.path.join(dsp, "FastMathFunctions", "arm_cos_f32.c"), os.path.join(dsp, "CommonTables", "arm_common_tables.c"),
            os.path.join(dsp, "BasicMathFunctions", "arm_scale_f32.c"), os.path.join(dsp, "BasicMathFunctions", "arm_add_f32.c")]
    q15 = os.path.join(dsp, "SupportFunctions", "arm_float_to_q15.c")
    flags = ["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-w", "-DARM_MATH_CM4"] + inc
    S = streams()
    out = {"names": np.array(sorted(S))}
    with tempfile.TemporaryDirectory() as tmp:
        h = os.path.join(tmp, "harness.c")
        with open(h, "w") as f:
            f.write(HARNESS)
        so, so_r = os.path.join(tmp, "libtxfm.so"), os.path.join(tmp, "libq15r.so")
        subprocess.run(flags + ["-shared", "-o", so, h, q15] + srcs + ["-lm"], check=True)
        subprocess.run(flags + ["-DARM_MATH_ROUNDING", "-shared", "-o", so_r, q15], check=True)      # the ARM_MATH_ROUNDING build of arm_float_to_q15
        L, R = C.CDLL(so), C.CDLL(so_r)
        vp = C.c_void_p
        L.txfm_run.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp, vp]
        L.txfm_run.restype = C.c_uint32
        R.arm_float_to_q15.argtypes = [vp, vp, C.c_uint32]
        R.arm_float_to_q15.restype = None
        for name, s in S.items():
            u = np.ascontiguousarray(s["u"], f32)
            assert u.shape == (N,) and np.isfinite(u).all()
            par = np.array([s["deviation"], s["amplitude"], s["tone_level"]], f32)
            ipar = np.array([s["step"], s["phase0"], s["tone_on"], s["tone_step"], s["tone_phase0"]], np.uint32)
            d, ph, o = np.zeros(N, np.int32), np.zeros(N, np.uint32), np.zeros((N, 2), f32)
            q0, q1 = np.zeros((N, 2), np.int16), np.zeros((N, 2), np.int16)
            tp = L.txfm_run(N, u.ctypes.data, par.ctypes.data, ipar.ctypes.data, d.ctypes.data, ph.ctypes.data, o.ctypes.data, q0.ctypes.data)
            R.arm_float_to_q15(o.ctypes.data, q1.ctypes.data, 2 * N)
            assert np.isfinite(o).all()
            for k, v in dict(u=u, par=par, ipar=ipar, d=d, phase=ph, out=o, q15_trunc=q0, q15_round=q1, tone_phase=np.uint32(tp)).items():
                out[name + "/" + k] = v
    # what the issue asks the streams to hold
    assert (out["saturate/d"] == 0x7FFFFFFF).any() and (out["saturate/d"] == -0x80000000).any()
    assert ((out["negfrac/d"] < 0) & (out["negfrac/d"] > -40)).any()
    wraps = np.diff(out["speech_t/phase"].astype(np.int64)) < 0
    assert wraps.sum() >= 3
    assert not np.array_equal(out["speech/q15_trunc"], out["speech/q15_round"])
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
