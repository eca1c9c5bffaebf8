"""CPU: the restatement of the audio output stage (tests/out_oracle.py, its C form over orc_fir_interpolate_f32 and its vectorised numpy
form) equals the reference's arm_fir_interpolate_f32 + arm_float_to_q15 bit for bit -- output and final state -- on
tests/golden/out_stage.npz (written by tests/golden/make_out_golden.py from the reference's own code), and the live reference where
oracle/_ref is built."""
import os

import numpy as np
import pytest

import out_oracle as oo
import rxcommon as rc

GOLDEN = np.load(os.path.join(rc.GOLDEN_DIR, "out_stage.npz"))
CASES = [str(c) for c in GOLDEN["cases"]]
CUTS = {str(n): GOLDEN["cut/" + str(n)].tolist() for n in GOLDEN["cut_names"]}


def _case(name):
    return {k.split("/", 1)[1]: GOLDEN[k] for k in GOLDEN.files if k.startswith(name + "/")}


def _run(g, lens, form, na=None):
    st = oo.OutStage(1, int(g["interp"]), g["coeffs"])
    ys, at = [], 0
    for n in lens:
        x = g["src"][None, at:at + n]
        ys.append(st.interp_np(x)[0] if form == "np" else st.interp_c(x, na if na and n % na == 0 else n)[0])
        at += n
    return np.concatenate(ys), st.state[0]


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_reference(name):
    g = _case(name)
    for cut, lens in CUTS.items():
        for form in ("c", "np"):
            y, state = _run(g, lens, form)
            assert y.tobytes() == g["y"].tobytes(), (cut, form)
            assert state.tobytes() == g["state"].tobytes(), (cut, form)
    # one call per DSP block of 24 inside longer calls: the composition the chain oracle uses
    y, state = _run(g, [96, 48, 48], "c", na=24)
    assert y.tobytes() == g["y"].tobytes() and state.tobytes() == g["state"].tobytes()
    # arm_float_to_q15, as the firmware builds it and with ARM_MATH_ROUNDING, and the stereo pair
    st = oo.OutStage(1, int(g["interp"]), g["coeffs"], oo.OUT_STEREO)
    for rounding, key in ((False, "q_trunc"), (True, "q_round")):
        q = st.format(g["y"][None, :], q15=True, rounding=rounding)[0]
        assert q.dtype == np.int16 and q[0::2].tobytes() == q[1::2].tobytes()
        # (outside the int32 range the reference's cast is undefined in C: there the FPU's saturation by sign, as oracle/rx_oracle.c states it)
        ok = g["q_defined"]
        want = np.where(ok, g[key], np.where(g["y"] > 0, 32767, -32768)).astype(np.int16)
        assert q[0::2].tobytes() == want.tobytes()
    f = st.format(g["y"][None, :])[0]
    assert f[0::2].tobytes() == g["y"].tobytes() and f[1::2].tobytes() == g["y"].tobytes()
    if rc.ref_available():
        _check_live_reference(name)


def test_fixture_covers_the_issue_cases():
    cases = {c: _case(c) for c in CASES}
    assert {int(g["interp"]) for g in cases.values()} == {1, 2, 4, 8}
    assert {g["coeffs"].size // int(g["interp"]) for g in cases.values()} == {1, 3, 8, 13, 64}
    assert len(cases) == 4 * 5 * 3
    assert CUTS["b24"] == [24] * 8 and CUTS["b64"] == [64] * 3 and len(CUTS["one"]) == 1 and min(CUTS["uneven"]) == 1
    assert any(0 < np.abs(g["src"]).max() < 1e-21 and g["y"].any() for g in cases.values())          # level 1e-22
    assert any(1e17 < np.abs(g["src"]).max() < 1e20 and np.isfinite(g["y"]).all() for g in cases.values())
    for g in cases.values():                                                                           # saturation hit on purpose, both ways
        if 0.5 < np.abs(g["src"]).max() < 10 and g["coeffs"].size // int(g["interp"]) >= 3:
            assert g["q_trunc"].max() == 32767 and g["q_trunc"].min() == -32768
    assert any((g["q_trunc"] != g["q_round"]).any() for g in cases.values())
    assert all(g["q_defined"].all() for g in cases.values() if np.abs(g["src"]).max() < 10)


def test_forms_agree_on_many_channels_and_blocks():
    """the C form (per channel and DSP block) and the numpy form (everything at once) on a batch, over several calls"""
    rng = np.random.default_rng(11)
    coeffs = rng.standard_normal(4 * 13).astype(np.float32)
    a, b = oo.OutStage(5, 4, coeffs, oo.OUT_STEREO), oo.OutStage(5, 4, coeffs, oo.OUT_STEREO)
    for n in (24, 48, 240):
        x = rng.standard_normal((5, n)).astype(np.float32)
        for q15 in (False, True):
            a2, b2 = oo.OutStage(5, 4, coeffs, oo.OUT_STEREO), oo.OutStage(5, 4, coeffs, oo.OUT_STEREO)
            a2.state, b2.state = a.state.copy(), b.state.copy()
            assert a2.process(x, 24, q15=q15, rounding=True, form="c").tobytes() == b2.process(x, q15=q15, rounding=True, form="np").tobytes()
        ya, yb = a.process(x, 24, form="c"), b.process(x, form="np")
        assert ya.shape == (5, n * 8) and ya.tobytes() == yb.tobytes() and a.state.tobytes() == b.state.tobytes()


def test_frames_only_passes_the_samples():
    x = np.array([[-0.0, 1.5, -2.0, 3e-40]], np.float32)
    st = oo.OutStage(1, 1, None, oo.OUT_STEREO)
    for form in ("c", "np"):
        assert st.process(x, form=form).tobytes() == np.repeat(x, 2, axis=1).tobytes()


def _check_live_reference(name):
    """where oracle/_ref is built: ref_fir_interpolate (the real arm_fir_interpolate_f32) on the same calls; elsewhere the fixture stands in"""
    import ctypes as C
    L = rc.ref_lib()
    L.ref_fir_interpolate.argtypes = [rc.f32p, C.c_uint32, C.c_uint32, rc.f32p, rc.f32p, rc.f32p, C.c_uint32]
    L.ref_fir_interpolate.restype = None
    g = _case(name)
    interp, coeffs = int(g["interp"]), g["coeffs"]
    P = coeffs.size // interp
    for lens in CUTS.values():
        state, ys, at = np.zeros(P - 1 + max(lens), np.float32), [], 0
        for n in lens:
            src, dst = np.ascontiguousarray(g["src"][at:at + n]), np.empty(n * interp, np.float32)
            L.ref_fir_interpolate(rc.fptr(coeffs), coeffs.size, interp, rc.fptr(state), rc.fptr(src), rc.fptr(dst), n)
            ys.append(dst); at += n
        y, st = _run(g, lens, "c")
        assert np.concatenate(ys).tobytes() == y.tobytes() and state[:P - 1].tobytes() == st.tobytes()
