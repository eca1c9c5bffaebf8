"""Writes tests/golden/txin.npz: the audio input stage of the TX chain (include/selenite_tx_in.h, DESIGN.md section 2 "TX input") composed of
the reference's CMSIS-DSP 1.5.3 functions -- arm_q15_to_float for int16 frames, arm_add_f32 and arm_scale_f32 for the MIX pick, arm_scale_f32
for the mic gain, arm_fir_decimate_f32 (+ init), arm_power_f32 for the VOX, arm_float_to_q15 (the truncating build and the
ARM_MATH_ROUNDING build) for the int16 chain -- for the numpy restatement in tests/txin_oracle.py (tests/test_txin_oracle.py checks it bit
for bit against this file) and for the kernel itself (tests/test_gpu_txin.py builds an instance from each stream's parameters).

One channel per stream, at most 512 outputs, the decimator from zero state, seeded; the harness runs DSP block by DSP block.  Streams:
  left     M = 4, 64 taps, int16 stereo frames, LEFT, DSP blocks of 64
  mix      M = 2, 97 unsymmetric taps of both signs, f32 stereo frames, MIX; frames that hold +-32768-scale values among ordinary ones and a
           gain that saturates arm_float_to_q15 at both ends; DSP blocks of 32
  mono8    M = 8, 256 taps, int16 mono frames, MONO, DSP blocks of 8: every block (64 inputs) is shorter than the history (255)
  right    M = 1, nd_taps = 0 (no FIR: a = g, a -0.0f stays -0.0f), f32 stereo frames, RIGHT, DSP blocks of 16
  vox      M = 2, 16 taps, f32 mono frames, DSP blocks of 8, hang = 2: bursts with gaps whose closing runs are shorter than, equal to and
           longer than hang; the level opens twice and closes twice (asserted below)
Kept per stream: frames, coeffs, par = {gain, attack, decay, open_level, close_level, level_init}, ipar = {M, pick, block, hang}, x (the
frame words as f32), g, a, both int16 builds of a, and per DSP block pw (arm_power_f32), level, open, hold, opens, open_blocks.  The law
behind arm_power_f32 is not a CMSIS function; the harness states it in C as the header does.

The reference files and the small harness below are compiled into a temporary directory with oracle/Makefile's flags (-std=gnu11 -O2
-ffp-contract=off -DARM_MATH_CM4), run, and deleted: nothing compiled is kept, and no test or build step compiles reference code.  Run by
hand where the reference tree is:
    python3 tests/golden/make_txin_golden.py REFERENCE_ROOT      (the root of the reference firmware tree)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "txin.npz")

HARNESS = r"""
#include <float.h>
#include <stdlib.h>
#include <string.h>
#include "arm_math.h"
/* one stream, DSP block by DSP block as DESIGN.md section 2 writes the input stage; par = {gain, attack, decay, open_level, close_level,
 * level_init}, ipar = {M, pick (0 MONO, 1 LEFT, 2 RIGHT, 3 MIX), block, hang, frames are int16} */
int txin_run(int N, const void *frames, int nt, const float *coeffs, const float *par, const uint32_t *ipar, float *x, float *g, float *a,
             int16_t *q15, float *pw, float *level, uint32_t *open, uint32_t *hold, uint64_t *opens, uint64_t *open_blocks)
{
    const uint32_t M = ipar[0], pick = ipar[1], nb = ipar[2], hang = ipar[3], isq = ipar[4], fw = pick == 0 ? 1 : 2, ni = nb * M;
    arm_fir_decimate_instance_f32 D;
    float *ds = calloc(nt + ni, sizeof(float)), *l = malloc(ni * sizeof(float)), *r = malloc(ni * sizeof(float)), *s = malloc(ni * sizeof(float));
    float lev = par[5];
    uint32_t op = 0, hd = 0;
    uint64_t ops = 0, obl = 0;
    if (nt && arm_fir_decimate_init_f32(&D, nt, M, (float *)coeffs, ds, ni) != ARM_MATH_SUCCESS) return 1;
    for (int b = 0; b < N / (int)nb; ++b) {
        const size_t w0 = (size_t)b * ni * fw;                     /* first frame word of the block */
        float *xb = x + w0, *gb = g + (size_t)b * ni, *ab = a + (size_t)b * nb;
        if (isq) arm_q15_to_float((q15_t *)frames + w0, xb, ni * fw);
        else memcpy(xb, (const float *)frames + w0, ni * fw * sizeof(float));
        if (pick == 0) memcpy(s, xb, ni * sizeof(float));
        else {
            for (uint32_t i = 0; i < ni; ++i) { l[i] = xb[2 * i]; r[i] = xb[2 * i + 1]; }
            if (pick == 1) memcpy(s, l, ni * sizeof(float));
            else if (pick == 2) memcpy(s, r, ni * sizeof(float));
            else { arm_add_f32(l, r, s, ni); arm_scale_f32(s, 0.5f, s, ni); }
        }
        arm_scale_f32(s, par[0], gb, ni);
        if (nt) arm_fir_decimate_f32(&D, gb, ab, ni);
        else memcpy(ab, gb, nb * sizeof(float));
        arm_power_f32(ab, nb, pw + b);
        {
            const float ms = pw[b] / (float)nb;
            if (ms <= FLT_MAX) {
                const float rr = ms > lev ? par[1] : par[2];
                const float d = ms - lev;
                lev = lev + rr * d;
            }
            if (!op) { if (lev > par[3]) { op = 1; hd = hang; ops += 1; } }
            else if (lev < par[4]) { if (hd == 0) op = 0; else hd -= 1; }
            else hd = hang;
            obl += op;
        }
        level[b] = lev; open[b] = op; hold[b] = hd; opens[b] = ops; open_blocks[b] = obl;
    }
    arm_float_to_q15(a, q15, (uint32_t)N);
    free(ds); free(l); free(r); free(s);
    return 0;
}
"""

SEED = 0x5458494E
f32 = np.float32
MONO, LEFT, RIGHT, MIX = 0, 1, 2, 3
VOX_OFF = dict(attack=0.5, decay=0.125, open_level=1e-6, close_level=5e-7, level_init=0.0, hang=0)


def lowpass(n, M):
    """a windowed-sinc decimation low-pass of gain 1 (any finite taps serve: they are stored in the fixture)"""
    k = np.arange(n, dtype=np.float64) - (n - 1) / 2
    h = np.sinc(0.8 * k / M) * np.hamming(n)
    return (h / h.sum()).astype(f32)


def streams():
    rng = np.random.default_rng(SEED)
    S = {}

    def q15(n):
        v = rng.integers(-30000, 30000, n).astype(np.int16)
        v[:6] = [32767, -32768, 0, -1, 1, -32767]
        return v
    S["left"] = dict(M=4, pick=LEFT, block=64, N=128, coeffs=lowpass(64, 4), gain=0.75, frames=q15(128 * 4 * 2), **VOX_OFF)
    fm = rng.uniform(-1, 1, 128 * 2 * 2).astype(f32)
    fm[40:48] = [32768.0, -32768.0, 32767.0, -32767.0, 32768.0, 32768.0, -32768.0, -32768.0]
    fm[300:304] = [-32768.0, 32767.0, 3.0, -3.0]
    S["mix"] = dict(M=2, pick=MIX, block=32, N=128, coeffs=(rng.uniform(-1, 1, 97) / 8).astype(f32), gain=2.5, frames=fm, **VOX_OFF)
    S["mono8"] = dict(M=8, pick=MONO, block=8, N=64, coeffs=lowpass(256, 8), gain=1.0, frames=q15(64 * 8), **VOX_OFF)
    fr = rng.uniform(-1, 1, 64 * 2).astype(f32)
    fr[1], fr[3], fr[5] = -0.0, 0.0, f32(1e-41)                     # RIGHT words: a signed zero and a denormal pass as they are
    S["right"] = dict(M=1, pick=RIGHT, block=16, N=64, coeffs=np.zeros(0, f32), gain=1.0, frames=fr, **VOX_OFF)
    # bursts of 4 DSP blocks at 0.5, quiet 1e-3 between them: gaps of 3, 4 and 9 blocks, then a burst and quiet to the end
    nb, M = 8, 2
    amp = np.full(64, 1e-3)
    at = 0
    for gap in (3, 4, 9, 30):
        amp[at:at + 4] = 0.5
        at += 4 + gap
    env = np.repeat(amp, nb * M)
    S["vox"] = dict(M=M, pick=MONO, block=nb, N=512, coeffs=lowpass(16, 2), gain=1.0, frames=(rng.uniform(-1, 1, env.size) * env).astype(f32),
                    attack=0.75, decay=0.875, open_level=2e-3, close_level=1e-3, level_init=0.0, hang=2)
    return S


def closing_runs(level, opened, close_level):
    """lengths of the runs of consecutive blocks with level < close_level that begin while the gate is open"""
    runs, n, was_open = [], 0, 0
    for lv, op in zip(level, opened):
        if lv < close_level and (n or was_open):
            n += 1
        elif n:
            runs.append(n)
            n = 0
        was_open = op
    if n:
        runs.append(n)
    return runs


def main(ref_root):
    dsp = os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Source")
    inc = ["-I" + os.path.join(ref_root, "Drivers", "CMSIS", "DSP", "Include"), "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Core", "Include"),
           "-I" + os.path.join(ref_root, "Drivers", "CMSIS", "Include")]
    names = ["SupportFunctions/arm_q15_to_float.c", "BasicMathFunctions/arm_add_f32.c", "BasicMathFunctions/arm_scale_f32.c",
             "FilteringFunctions/arm_fir_decimate_f32.c", "FilteringFunctions/arm_fir_decimate_init_f32.c", "StatisticsFunctions/arm_power_f32.c"]
    srcs = [os.path.join(dsp, *n.split("/")) for n in names]
    q15 = os.path.join(dsp, "SupportFunctions", "arm_float_to_q15.c")
    flags = ["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-w", "-DARM_MATH_CM4"] + inc
    S = streams()
    out = {"names": np.array(sorted(S))}
    with tempfile.TemporaryDirectory() as tmp:
        h = os.path.join(tmp, "harness.c")
        with open(h, "w") as f:
            f.write(HARNESS)
        so, so_r = os.path.join(tmp, "libtxin.so"), os.path.join(tmp, "libtxin_r.so")
        subprocess.run(flags + ["-shared", "-o", so, h, q15] + srcs + ["-lm"], check=True)
        subprocess.run(flags + ["-DARM_MATH_ROUNDING", "-shared", "-o", so_r, h, q15] + srcs + ["-lm"], check=True)   # arm_float_to_q15's other build
        vp = C.c_void_p
        libs = []
        for path in (so, so_r):
            L_ = C.CDLL(path)
            L_.txin_run.argtypes = [C.c_int, vp, C.c_int] + [vp] * 13
            libs.append(L_)
        for name, s in S.items():
            frames = np.ascontiguousarray(s["frames"])
            N, M, nb, fw = s["N"], s["M"], s["block"], 1 if s["pick"] == MONO else 2
            assert N <= 512 and N % nb == 0 and frames.size == N * M * fw and frames.dtype in (np.float32, np.int16)
            coeffs = np.ascontiguousarray(s["coeffs"], f32)
            assert np.isfinite(coeffs).all()
            par = np.array([s["gain"], s["attack"], s["decay"], s["open_level"], s["close_level"], s["level_init"]], f32)
            ipar = np.array([M, s["pick"], nb, s["hang"], int(frames.dtype == np.int16)], np.uint32)
            nblk = N // nb
            res = {}
            for tag, L_ in zip(("trunc", "round"), libs):
                x, g, a, q = np.zeros(frames.size, f32), np.zeros(N * M, f32), np.zeros(N, f32), np.zeros(N, np.int16)
                pw, level = np.zeros(nblk, f32), np.zeros(nblk, f32)
                opn, hold = np.zeros(nblk, np.uint32), np.zeros(nblk, np.uint32)
                opens, oblk = np.zeros(nblk, np.uint64), np.zeros(nblk, np.uint64)
                rc_ = L_.txin_run(N, frames.ctypes.data, coeffs.size, coeffs.ctypes.data if coeffs.size else None, par.ctypes.data, ipar.ctypes.data,
                                  x.ctypes.data, g.ctypes.data, a.ctypes.data, q.ctypes.data, pw.ctypes.data, level.ctypes.data, opn.ctypes.data,
                                  hold.ctypes.data, opens.ctypes.data, oblk.ctypes.data)
                assert rc_ == 0 and np.isfinite(a).all()
                res[tag] = dict(x=x, g=g, a=a, q15=q, pw=pw, level=level, open=opn, hold=hold, opens=opens, open_blocks=oblk)
            for k_ in ("x", "g", "a", "pw", "level", "open", "hold", "opens", "open_blocks"):      # the f32 path does not depend on the q15 build
                assert res["trunc"][k_].tobytes() == res["round"][k_].tobytes()
                out[name + "/" + k_] = res["trunc"][k_]
            out[name + "/q15_trunc"], out[name + "/q15_round"] = res["trunc"]["q15"], res["round"]["q15"]
            for k_, v in dict(frames=frames, coeffs=coeffs, par=par, ipar=ipar).items():
                out[name + "/" + k_] = v
    # what the issue asks the fixture to hold
    assert (out["mix/q15_trunc"] == 32767).any() and (out["mix/q15_trunc"] == -32768).any()
    assert not np.array_equal(out["left/q15_trunc"], out["left/q15_round"])
    assert (np.abs(out["mix/frames"]) >= 32767).sum() >= 8 and (out["mix/coeffs"] > 0).any() and (out["mix/coeffs"] < 0).any()
    assert not np.array_equal(out["mix/coeffs"], out["mix/coeffs"][::-1])
    assert out["right/a"].tobytes() == np.ascontiguousarray(out["right/frames"][1::2]).tobytes() and np.signbit(out["right/a"][0])
    assert out["mono8/ipar"][2] * out["mono8/ipar"][0] < out["mono8/coeffs"].size - 1
    op, hang = out["vox/open"], int(out["vox/ipar"][3])
    rises = int(((op[1:] == 1) & (op[:-1] == 0)).sum()) + int(op[0])
    falls = int(((op[1:] == 0) & (op[:-1] == 1)).sum())
    runs = closing_runs(out["vox/level"], op, out["vox/par"][4])
    print("vox: opens %d, closes %d, closing runs %s, hang %d" % (rises, falls, runs, hang))
    assert rises >= 2 and falls >= 2 and int(out["vox/opens"][-1]) == rises
    assert any(r < hang for r in runs) and any(r == hang for r in runs) and any(r > hang for r in runs)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
