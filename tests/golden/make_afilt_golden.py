"""Writes tests/golden/afilt.npz: arm_biquad_cascade_df1_f32 of the reference's CMSIS-DSP 1.5.3, through the existing ref_biquad of
oracle/_ref/libcmsis_ref.so (rxcommon.RefLib.biquad), for the numpy restatement of the audio filter stage in tests/afilt_oracle.py
(tests/test_afilt_oracle.py checks it bit for bit against this file) and for the stage itself (tests/test_gpu_afilt.py).

Per n_stages = 1 .. 8 three streams ("channels"), each cut into calls of 1, 3, 4, 12, 24, 96 and 256 samples on one running state (the
reference's loop unrolled by 4 and its tail both run):
  0  sections from the design helpers (notch, peaking, low-pass, high-pass, de-emphasis in turn), noise and a tone
  1  random stable pole pairs, noise with -0.0f and denormals in it
  2  random stable pole pairs, noise with +-FLT_MAX in the call of 96 and +-Inf in the call of 256 (the state goes NaN and stays NaN)
Data only: nothing compiled is kept.  Run by hand where oracle/_ref is built (the build does that where the reference sources are):
    python3 tests/golden/make_afilt_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rxcommon as rc  # noqa: E402
import selenite_rx as sr  # noqa: E402

OUT = os.path.join(HERE, "afilt.npz")
SEED = 0x4146494C
LENGTHS = (1, 3, 4, 12, 24, 96, 256)
FLT_MAX = np.finfo(np.float32).max


def designed(ns):
    """ns sections from the helpers, in turn"""
    secs = [sr.design_biquad(sr.BIQUAD_NOTCH, 1000.0 / 12000.0, 10.0), sr.design_biquad(sr.BIQUAD_PEAKING, 0.11, 2.0, 6.0),
            sr.design_biquad(sr.BIQUAD_LOWPASS, 0.22, 0.7071), sr.design_biquad(sr.BIQUAD_HIGHPASS, 0.02, 0.7071),
            sr.design_deemphasis(0.9), sr.design_biquad(sr.BIQUAD_PEAKING, 0.3, 1.0, -9.0), sr.design_biquad(sr.BIQUAD_NOTCH, 2300.0 / 12000.0, 30.0),
            sr.design_biquad(sr.BIQUAD_LOWPASS, 0.4, 1.5)]
    return np.stack(secs[:ns]).astype(np.float32)


def random_stable(ns, rng):
    """pole pairs r e^{+-j theta}, 0.5 < r < 0.99: a1 = 2 r cos theta, a2 = -r^2 in CMSIS sign; numerators in (-1, 1)"""
    r, th = rng.uniform(0.5, 0.99, ns), rng.uniform(0.05, 3.0, ns)
    c = np.empty((ns, 5))
    c[:, :3] = rng.uniform(-1, 1, (ns, 3))
    c[:, 3], c[:, 4] = 2 * r * np.cos(th), -r * r
    return c.astype(np.float32)


def main():
    ref = rc.RefLib()
    assert ref.live, "oracle/_ref/libcmsis_ref.so is not built here"
    rng = np.random.default_rng(SEED)
    total = sum(LENGTHS)
    starts = np.cumsum((0,) + LENGTHS[:-1])
    out = {"lengths": np.array(LENGTHS, np.int64)}
    for ns in range(1, 9):
        coeffs = np.stack([designed(ns), random_stable(ns, rng), random_stable(ns, rng)])
        t = np.arange(total)
        x = rng.uniform(-0.3, 0.3, (3, total))
        x[0] += 0.5 * np.cos(2 * np.pi * 0.0833 * t)
        x = x.astype(np.float32)
        x[1, rng.choice(total, 40, replace=False)] = np.float32(-0.0)
        den = rng.choice(total, 40, replace=False)
        x[1, den] = (rng.uniform(-1, 1, 40) * 1e-39).astype(np.float32)
        x[1, 0], x[1, 1] = np.float32(-0.0), np.float32(1e-42)
        a96, a256 = starts[5], starts[6]
        x[2, a96 + 7], x[2, a96 + 50] = FLT_MAX, -FLT_MAX
        x[2, a256 + 100], x[2, a256 + 180] = np.inf, -np.inf
        y = np.empty_like(x)
        states = np.zeros((len(LENGTHS), 3, ns, 4), np.float32)
        for c in range(3):
            st = np.zeros(4 * ns, np.float32)
            k5 = np.ascontiguousarray(coeffs[c].reshape(-1))
            for i, (a, n) in enumerate(zip(starts, LENGTHS)):
                y[c, a:a + n] = ref.biquad(k5, ns, st, np.ascontiguousarray(x[c, a:a + n]), n)
                states[i, c] = st.reshape(ns, 4)
        assert np.isfinite(y[:2]).all() and np.isnan(y[2, -1]) and np.isfinite(y[2, :a96]).all()
        out["ns%d/coeffs" % ns], out["ns%d/x" % ns], out["ns%d/y" % ns], out["ns%d/state" % ns] = coeffs, x, y, states
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
