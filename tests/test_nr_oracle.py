"""CPU: the numpy restatement of the NLMS stage (tests/nr_oracle.py) equals the reference's arm_lms_norm_f32 bit for bit
(tests/golden/lms_norm.npz, written by tests/golden/make_nr_golden.py from the reference's own code), and the stage does what it is for:
NOTCH takes a steady tone out, DENOISE raises a tone above white noise."""
import os

import numpy as np
import pytest

import nr_oracle as nro
import rxcommon as rc

GOLDEN = np.load(os.path.join(rc.GOLDEN_DIR, "lms_norm.npz"))


@pytest.mark.parametrize("name", [str(c) for c in GOLDEN["cases"]])
def test_restatement_equals_reference(name):
    g = {k.split("/", 1)[1]: GOLDEN[k] for k in GOLDEN.files if k.startswith(name + "/")}
    st = nro.Nlms(1, int(g["num_taps"]), float(g["mu"]), g["coeffs_init"])
    ys, es, at = [], [], 0
    for n in g["lens"]:
        y, e = st.lms(g["src"][None, at:at + n], g["ref"][None, at:at + n])
        ys.append(y[0]); es.append(e[0]); at += n
    assert np.concatenate(ys).tobytes() == g["y"].tobytes()
    assert np.concatenate(es).tobytes() == g["e"].tobytes()
    assert st.coeffs[0].tobytes() == g["coeffs"].tobytes()
    assert st.window[0].tobytes() == g["window"].tobytes()
    assert st.energy.tobytes() == g["energy"].tobytes() and st.x0.tobytes() == g["x0"].tobytes()


def test_fixture_covers_the_issue_cases():
    taps = {int(GOLDEN[c + "/num_taps"]) for c in GOLDEN["cases"]}
    mus = {float(GOLDEN[c + "/mu"]) for c in GOLDEN["cases"]}
    assert taps == {5, 8, 16, 32, 64}
    assert {0.01, 0.5, 1.5} <= {round(m, 6) for m in mus}
    assert any(len(GOLDEN[c + "/lens"]) == 7 for c in GOLDEN["cases"])
    # the edges of the arithmetic (tests/test_gpu_nr_edges.py rests on the restatement there)
    cases = {str(c): {k.split("/", 1)[1]: GOLDEN[k] for k in GOLDEN.files if k.startswith(str(c) + "/")} for c in GOLDEN["cases"]}
    tiny = np.finfo(np.float32).tiny
    gaps = [g for g in cases.values() if (g["ref"] == 0).sum() >= 200 and g["ref"][:100].any() and g["ref"][-100:].any()]
    assert {8, 64} <= {int(g["num_taps"]) for g in gaps}                                      # burst, exact silence, the signal back
    for g in gaps:                                                                            # ... with a negative energy when it comes back
        st = nro.Nlms(1, int(g["num_taps"]), float(g["mu"]), g["coeffs_init"])
        n = int(np.flatnonzero(g["ref"] == 0).max()) + 1                                      # (a call boundary: the generator's ("gap", a, b, L))
        assert n in np.cumsum(g["lens"]) and int(np.flatnonzero(g["ref"] == 0).min()) not in np.cumsum(g["lens"])
        st.lms(g["src"][None, :n], g["ref"][None, :n])
        assert st.energy[0] < 0 and not g["src"][n - int(g["num_taps"]) - 1:n].any()
    assert any(0 < abs(float(g["energy"][0])) < tiny for g in cases.values())                # a denormal energy (level 1e-22)
    assert any(1e17 < np.abs(g["ref"]).max() < 1e19 and np.isfinite(g["y"]).all() and np.isfinite(g["coeffs"]).all() for g in cases.values())
    assert any(len(g["lens"]) >= 30 and min(g["lens"]) == 1 and {12, 24, 36} <= set(g["lens"].tolist()) for g in cases.values())   # many short calls


def test_restatement_is_vectorised_per_channel():
    """channels are independent: a batch gives each row what it alone gives"""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 300)).astype(np.float32)
    batch = nro.Nlms(4, 16, 0.3, delay=5).process(x, nro.NR_NOTCH)
    for c in range(4):
        one = nro.Nlms(1, 16, 0.3, delay=5).process(x[c:c + 1], nro.NR_NOTCH)
        assert one.tobytes() == batch[c:c + 1].tobytes()


F_TONE = 0.125          # cycles per sample: a steady tone (a carrier, a heterodyne)


def _tone_and_noise(n=4000):
    rng = np.random.default_rng(0x70E)
    t = np.arange(n)
    tone = (np.sqrt(2.0) * np.sin(2 * np.pi * F_TONE * t)).astype(np.float32)     # power 1
    noise = (rng.standard_normal(n) * 10 ** (-17 / 20)).astype(np.float32)          # 17 dB below
    return tone, noise


def _tone_power(y, f=F_TONE):
    """power of the tone component (least-squares fit of a cosine and a sine at f)"""
    return float(np.mean(_tone_fit(y, f) ** 2))


def _tone_fit(y, f=F_TONE):
    t = np.arange(y.size)
    basis = np.stack([np.cos(2 * np.pi * f * t), np.sin(2 * np.pi * f * t)], axis=1)
    coef = np.linalg.lstsq(basis, y.astype(np.float64), rcond=None)[0]
    return basis @ coef


def test_notch_removes_a_steady_tone():
    tone, noise = _tone_and_noise()
    x = (tone + noise)[None, :]
    e = nro.Nlms(1, 32, 0.05, delay=16).process(x, nro.NR_NOTCH)[0]
    before, after = _tone_power(x[0, 2000:]), _tone_power(e[2000:])
    assert 10 * np.log10(before / after) >= 30.0


def test_denoise_raises_tone_to_noise():
    tone, noise = _tone_and_noise()
    x = (tone + noise)[None, :]
    y = nro.Nlms(1, 32, 0.05, delay=16).process(x, nro.NR_DENOISE)[0]

    def tnr(sig):
        fit = _tone_fit(sig)
        return float(np.mean(fit ** 2)) / float(np.mean((sig.astype(np.float64) - fit) ** 2))
    gain_db = 10 * np.log10(tnr(y[2000:]) / tnr(x[0, 2000:]))
    assert gain_db >= 5.0
