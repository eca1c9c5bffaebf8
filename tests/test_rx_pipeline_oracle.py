"""CPU: the composition of the RX stage oracles (tests/rx_pipeline_oracle.py: Pipeline) pinned to its parts -- each part is pinned to the
reference by a fixture of its own.  With one stage on the composition is that stage's oracle fed the oracle chain's audio; with none it is
rc.CpuChain with its AGC on (the chain-AGC-off + nr_oracle.Agc + float_to_q15 decomposition everything else rests on); it does not depend
on how the stream is cut; the split global-gain call is the one call; and on the fuzz input (tests/rx_stage_fuzz_cases.py: signal) a
wrong order of two stages changes bits, which is what gives the GPU comparison (tests/test_gpu_rx_stage_fuzz.py) its teeth."""
import numpy as np
import pytest

import afilt_oracle as ao
import cwdec_oracle as co
import iqc_oracle as io
import meter_oracle as mo
import nb_oracle as no
import nr_oracle as nro
import out_oracle as oo
import rx_pipeline_oracle as po
import rx_stage_fuzz_cases as fz
import rxcommon as rc
import spectrum_oracle as so
import tones_oracle as to

CH, BLOCKS = 5, 12
PAR = dict(
    spectrum=dict(fft_len=64, stride=2, average=1, alpha=0.25),
    iqc=dict(frame=64, alpha=0.25, dc_alpha=0.25, p_max=0.5, g_max=2.0, min_power=1e-10, p_init=0.02, g_init=0.97, dc_i_init=0.005, dc_q_init=0.0),
    nb=dict(frame=64, guard=2, max_hits=6, threshold=6.0, alpha=0.25, clamp=2.0),
    tones=dict(coeffs=to.design([0.05, 0.11, 0.2]), frame_blocks=2, confirm=1, release=1, ratio=0.0, min_power=1e-9),
    cwdec=dict(peak_attack=0.5, peak_decay=0.01, floor_attack=0.25, floor_decay=0.01, on_frac=0.4, off_frac=0.25, snr=4.0, min_power=1e-12,
               debounce=1, adapt=1, track=1, unit_min=256, unit_init=2 * 256, unit_max=16 * 256, ring=16),
    afilt=dict(coeffs=[fz._highpass(0.03, 0.7071), fz._notch(0.12, 4.0)], per_channel=False),
    nr=dict(kind=nro.NR_DENOISE, num_taps=8, delay=4, mu=0.2),
    meter=dict(sense=mo.ABOVE, gate=1, hang=1, attack=0.5, decay=0.9375, open_level=2e-4, close_level=4e-5, level_init=0.0),
    out=dict(interp=2, coeffs=rc.design_lowpass(16, 0.2) * np.float32(2.0), frames=oo.OUT_STEREO),
)
CASE = dict(spec=dict(channels=CH, block=256), signal_seed=12345)


def spec_of(**kw):
    kw.setdefault("agc", True)
    return rc.baseline_spec("cfg3", CH, kw.pop("arith", rc.ARITH_CMSIS), **kw)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.itemsize]
        bad = np.argwhere(got.view(u) != want.view(u))
        raise AssertionError("%s: %d of %d values differ, first at %s" % (what, len(bad), got.size, bad[0]))


def same_states(a, b, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for name in a:
        if isinstance(a[name], dict):
            assert set(a[name]) == set(b[name]), (what, name)
            for k in a[name]:
                same(a[name][k], b[name][k], "%s: %s.%s" % (what, name, k))
        else:
            same(a[name], b[name], "%s: %s" % (what, name))


@pytest.fixture(scope="module")
def iq():
    return fz.signal(CASE, 0, BLOCKS * 256)


@pytest.fixture(scope="module")
def audio(iq):
    """the oracle chain's un-scaled audio of the whole stream, computed once"""
    return rc.CpuChain(po.no_agc(spec_of()), "orc").process(iq)


def scaled(a, spec=None):
    spec = spec or spec_of()
    return nro.Agc(CH, 64, spec.agc_params, spec.agc_global).process(a)


# ---- one stage on ---------------------------------------------------------------------------------------------------------------------------
def test_spectrum_alone(iq):
    p, s = po.Pipeline(spec_of(), dict(spectrum=PAR["spectrum"])), so.Spectrum(CH, **PAR["spectrum"])
    for data in (iq[:, :768], fz.to_q15(iq[:, 768:2048])):
        got = p.process_audio(None, data)
        s.process(data)
        assert got.dtype == data.dtype
    same_states({"spectrum": s.state()}, {"spectrum": p.state()["spectrum"]}, "spectrum")
    assert p.spectrum_frames() == s.frames and s.rows.any()
    ref = rc.CpuChain(spec_of(), "orc")
    ref.process(iq[:, :768])
    same(got, ref.process_q15(fz.to_q15(iq[:, 768:2048])), "a tap changes no audio")


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_iqc_alone_and_nb_alone(iq, q15):
    data = fz.to_q15(iq) if q15 else iq
    for name, cls in (("iqc", io.Corrector), ("nb", no.Blanker)):
        p, s, ref = po.Pipeline(spec_of(), {name: PAR[name]}), cls(CH, **PAR[name]), rc.CpuChain(spec_of(), "orc")
        x = s.process(data)
        assert x.dtype == (np.int16 if q15 and name == "nb" else np.float32)        # the correction leaves f32, the blanker the caller's format
        a = ref.process(po.q15_to_float(x) if x.dtype == np.int16 else x)
        same(p.process_audio(None, data), nro.float_to_q15(a) if q15 else a, name)
        same_states({name: s.state()}, {name: p.state()[name]}, name)
        same_states({"chain": ref.state()}, {"chain": p.state()["chain"]}, name + ": chain")
    assert s.blanked.any()


@pytest.mark.parametrize("name", ["tones", "cwdec"])
def test_a_tap_alone(iq, audio, name):
    p = po.Pipeline(spec_of(), {name: PAR[name]})
    s = to.Tones(CH, 64, **PAR[name]) if name == "tones" else co.CwDec(CH, 64, **PAR[name])
    same(p.process(iq), scaled(audio), name + ": audio")
    s.process(audio)
    same_states({name: s.state()}, {name: p.state()[name]}, name)
    assert s.changes.any() if name == "tones" else s.count.any()


def test_afilt_alone_and_nr_alone(iq, audio):
    f = ao.Afilt(CH, **PAR["afilt"])
    p = po.Pipeline(spec_of(), dict(afilt=PAR["afilt"]))
    same(p.process(iq), scaled(f.process(audio)), "afilt")
    same(p.state()["afilt"]["state"], f.state, "afilt state")
    same(p.state()["afilt"]["coeffs"], np.array(PAR["afilt"]["coeffs"], np.float32), "afilt coeffs")
    n = nro.Nlms(CH, 8, 0.2, None, 4)
    p = po.Pipeline(spec_of(), dict(nr=PAR["nr"]))
    same(p.process(iq), scaled(n.process(audio, nro.NR_DENOISE)), "nr")
    same_states({"nr": n.state()}, {"nr": p.state()["nr"]}, "nr")
    assert n.coeffs.any()


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_meter_alone(iq, audio, q15):
    m = mo.Meter(CH, 64, **PAR["meter"])
    p = po.Pipeline(spec_of(), dict(meter=PAR["meter"]))
    if q15:
        data = fz.to_q15(iq)
        a = rc.CpuChain(po.no_agc(spec_of()), "orc").process(po.q15_to_float(data))
        bits = m.process(a)
        same(p.process_q15(data), m.gate_audio(nro.float_to_q15(scaled(a)), bits), "gated int16 words")
    else:
        bits = m.process(audio)
        same(p.process(iq), m.gate_audio(scaled(audio), bits), "gated audio")
    same_states({"meter": m.state()}, {"meter": p.state()["meter"]}, "meter")
    assert bits.any() and not bits.all()


# ---- no stage on ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounding", [False, True], ids=["trunc", "round"])
@pytest.mark.parametrize("agc", ["off", "channel", "global"])
@pytest.mark.parametrize("arith", [rc.ARITH_CMSIS, rc.ARITH_FMA], ids=["cmsis", "fma"])
def test_no_stage_is_the_chain_with_its_own_agc(iq, arith, agc, rounding):
    spec = spec_of(arith=arith, agc=agc != "off", agc_global=agc == "global", q15_rounding=rounding,
                   agc_params=fz.AGC_ODD if rounding else None)
    p, ref = po.Pipeline(spec), rc.CpuChain(spec, "orc")
    same(p.process(iq[:, :1024]), ref.process(iq[:, :1024]), "f32")
    q = fz.to_q15(iq[:, 1024:])
    same(p.process_q15(q), ref.process_q15(q), "int16")
    same_states({"chain": ref.state()}, p.state(), "chain state")


# ---- output stage only ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_out_alone_is_staged_chain(iq, q15):
    spec = spec_of(q15_rounding=True)
    p, ref = po.Pipeline(spec, dict(out=PAR["out"])), oo.StagedChain(spec, **PAR["out"])
    for a, b in ((0, 768), (768, 3072)):
        data = fz.to_q15(iq[:, a:b]) if q15 else iq[:, a:b]
        same(p.process_audio(None, data), ref.process_q15(data) if q15 else ref.process(data), "frames")
    same(p.state()["out"], ref.stage.state, "interpolator history")


# ---- cut invariance, the split call -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_every_stage_on_one_call_equals_calls_of_1_3_and_the_rest(iq, q15):
    data = fz.to_q15(iq) if q15 else iq
    one, cut = po.Pipeline(spec_of(), PAR), po.Pipeline(spec_of(), PAR)
    whole = one.process_audio(None, data)
    parts = [cut.process_audio(None, data[:, a * 256:b * 256]) for a, b in ((0, 1), (1, 4), (4, BLOCKS))]
    same(np.concatenate(parts, axis=1), whole, "frames")
    same_states(one.state(), cut.state(), "states")
    assert set(one.state()) == set(po.STAGES) | {"chain"}
    assert one.spectrum_frames() == cut.spectrum_frames()


def test_split_call_equals_one_call(iq):
    stages = {k: v for k, v in PAR.items() if k != "out"}
    spec = spec_of(agc_global=True)
    one, two = po.Pipeline(spec, stages), po.Pipeline(spec, stages)
    for a, b in ((0, 1024), (1024, 3072)):
        want = one.process(iq[:, a:b])
        pre, env = two.phase1(iq[:, a:b])
        mid = two.state()
        assert env.shape == ((b - a) // 256,) and env.dtype == np.float32
        same(env, np.abs(pre).reshape(CH, -1, 64).max(axis=(0, 2)), "envelope row")
        same(two.phase2(), want, "audio")
        after = two.state()
        for name in stages:                                          # phase 2 runs the gain and the gate, nothing else
            same_states({name: mid[name]}, {name: after[name]}, "phase 2 moved " + name)
    same_states(one.state(), two.state(), "states")
    # the envelope handed to phase 2 is the one phase 1 returned
    three = po.Pipeline(spec, stages)
    pre, env = three.phase1(iq[:, :1024])
    same(three.phase2(env), po.Pipeline(spec, stages).process(iq[:, :1024]), "phase 2 with the row of phase 1")


# ---- life cycle ---------------------------------------------------------------------------------------------------------------------------------
def test_state_round_trip_reset_set_mode_and_set_stage(iq):
    a = po.Pipeline(spec_of(), PAR)
    a.process(iq[:, :1280])
    b = po.Pipeline(spec_of(), PAR)
    b.set_state(a.state())
    same_states(a.state(), b.state(), "restored")
    same(a.process(iq[:, 1280:2048]), b.process(iq[:, 1280:2048]), "the call behind the restore")
    same_states(a.state(), b.state(), "behind the call")
    a.reset()
    same_states(a.state(), po.Pipeline(spec_of(), PAR).state(), "reset")
    same(a.process(iq[:, :1280]), po.Pipeline(spec_of(), PAR).process(iq[:, :1280]), "the same stream behind reset")
    # set_mode moves the chain and no stage; the mode survives reset
    before = a.state()
    assert a.set_mode(rc.MODE_LSB) == 0
    same_states(before, a.state(), "set_mode")
    a.reset()
    lsb = spec_of()
    lsb.mode = rc.MODE_LSB
    same(a.process(iq[:, :512]), po.Pipeline(lsb, PAR).process(iq[:, :512]), "LSB behind reset")
    # a stage removed is no stage; set again it starts fresh, the others keep their state
    a.set_stage("afilt", None)
    assert "afilt" not in a.state()
    keep = a.state()["nr"]
    a.set_stage("afilt", PAR["afilt"])
    assert not a.state()["afilt"]["state"].any()
    same_states({"nr": keep}, {"nr": a.state()["nr"]}, "nr across set_afilt")


# ---- the order is observable on the fuzz input -----------------------------------------------------------------------------------------------------
def differs(a, b):
    return np.asarray(a).tobytes() != np.asarray(b).tobytes()


def test_order_matters_on_the_fuzz_input(iq):
    spec = spec_of()
    on = {k: PAR[k] for k in ("tones", "cwdec", "afilt", "nr", "meter")}
    right = po.Pipeline(spec, on)
    y = right.process(iq)
    st = right.state()
    # NLMS in front of the audio filter
    wrong = po.Pipeline(spec, on)
    wrong.order = ("tones", "cwdec", "nr", "afilt", "meter")
    assert differs(wrong.process(iq), y) and differs(wrong.state()["nr"]["coeffs"], st["nr"]["coeffs"])
    # the taps behind the filter
    wrong = po.Pipeline(spec, on)
    wrong.order = ("afilt", "tones", "cwdec", "nr", "meter")
    assert not differs(wrong.process(iq), y), "a tap changes no audio wherever it reads"
    ws = wrong.state()
    assert differs(ws["tones"]["power"], st["tones"]["power"]) and differs(ws["tones"]["frame_energy"], st["tones"]["frame_energy"])
    assert differs(ws["cwdec"]["peak"], st["cwdec"]["peak"]) and differs(ws["cwdec"]["floor"], st["cwdec"]["floor"])
    # the gate in front of the AGC: the AGC then sees silent blocks
    wrong = po.Pipeline(spec, on)
    wrong.gate_first = True
    wrong.process(iq)
    assert differs(wrong.state()["chain"]["agc_gain"], st["chain"]["agc_gain"])
    m = st["meter"]
    assert m["opens"].any() and (m["open_blocks"] < BLOCKS).any(), "the gate was open on some blocks and closed on others"
