"""CPU: the AGC / ALC gain law at non-default parameters (tests/gain_law_cases.py: SETS and the level plan).  The oracle's orc_agc_update,
the whole RX oracle chain (per channel and agc_global, f32 and int16 slots) and the TX oracle with its ALC are compared on bits with the
numpy restatement nr_oracle.Agc applied to the oracle's own un-scaled audio (AGC / ALC off).

The coverage and sensitivity conditions are asserted here, on the restatement alone, for every shape and channel count that
tests/test_gpu_gain_law.py runs -- so that a GPU case cannot go hollow: over its six calls the set `odd` meets the floor, both clamps and
both branches, `fast` has blocks with d - g == 0, `slow` meets attack, decay and the upper clamp; and a restatement with target * (1 / e) in
place of the division, one with the update fused (f64, rounded once) and one on the default parameters each differ in bits from the true one
(`fast` cannot show the fused update: rate 1.0)."""
import ctypes as C
import functools

import numpy as np
import pytest

import gain_law_cases as gl
import nr_oracle as nro
import rxcommon as rc

f32 = np.float32


@functools.lru_cache(maxsize=None)
def unscaled(shape, channels, q15=False, rows=None, plain=False):
    """the CMSIS oracle chain's audio of the six calls with its AGC off (no parameter of the law touches it): [(input, audio f32)]"""
    spec = gl.rx_spec(shape, channels, rc.ARITH_CMSIS, gl.RX_DEFAULTS, agc=False)
    orc = rc.CpuChain(spec, "orc")
    assert orc.ok()
    out = []
    for x in gl.rx_plan(shape, channels, q15, rows, plain):
        out.append((x, orc.process(gl.q15_to_f32(x) if q15 else x)))
    return spec.block // spec.decim, out


# ---- 1. the law itself ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_orc_agc_update_equals_the_restatement(oracle, name):
    """orc_agc_update, one call per (gain, env), against one step of nr_oracle.Agc: envelopes over 10^-8 ... 10^3, exact zero (floor 0:
    target / 0 = +inf -> gain_max), the floor itself and both clamp edges; gains across [gain_min, gain_max]"""
    p = gl.SETS[name]
    rng = np.random.default_rng(11)
    env = (10.0 ** rng.uniform(-8, 3, 4096)).astype(f32)
    env[:8] = [0.0, p["env_floor"], p["target"] / p["gain_max"], p["target"] / p["gain_min"], 1.0, 0.5, np.nextafter(f32(p["env_floor"]), f32(0)), 1e-30]
    gain = (10.0 ** rng.uniform(np.log10(p["gain_min"]), np.log10(p["gain_max"]), env.size)).astype(f32)
    gain[:4] = [p["gain_init"], p["gain_min"], p["gain_max"], 1.0]
    cfg = rc.ChainSpec(1, 4, agc_params=p).config()
    got = np.array([oracle.orc_agc_update(C.byref(cfg), C.c_float(g), C.c_float(e), 0) for g, e in zip(gain, env)], f32)
    law = nro.Agc(env.size, 1, p)
    law.gain = gain.copy()
    law.process(env.reshape(-1, 1))
    gl.assert_bits(got, law.gain, name)
    # the restatement on block maxima (what the conditions below are computed from) is the same statement
    gl.assert_bits(gl.law_trace(env.reshape(1, -1), p)[0], nro_run(env, p), name + ": law_trace")


def nro_run(env, p):
    law, out = nro.Agc(1, 1, p), []
    for e in env:
        law.process(np.array([[e]], f32))
        out.append(law.gain[0])
    return np.array(out, f32).reshape(1, -1)


# ---- 2. the RX oracle chain, every shape and channel count of the GPU test, with the conditions -------------------------------------------
@pytest.mark.parametrize("channels", gl.CHANNELS)
@pytest.mark.parametrize("name,shape", gl.RX_RUNS)
def test_rx_oracle_chain_equals_the_restatement(name, shape, channels):
    """CpuChain(spec, "orc") with the AGC on == nr_oracle.Agc of the same chain's AGC-off audio: audio of every call and the final agc_gain,
    on bits; every other row of the state equal to the AGC-off chain's.  The conditions hold on this run's block maxima."""
    na, calls = unscaled(shape, channels)
    spec = gl.rx_spec(shape, channels, rc.ARITH_CMSIS, gl.SETS[name])
    orc, law = rc.CpuChain(spec, "orc"), nro.Agc(channels, na, gl.SETS[name])
    assert orc.ok()
    for i, (iq, pre) in enumerate(calls):
        gl.assert_bits(orc.process(iq), law.process(pre), "%s %s call %d" % (name, shape, i))
    gl.assert_bits(orc.state()["agc_gain"], law.gain, "agc_gain")
    env = np.concatenate([gl.block_maxima(pre, na) for _, pre in calls], axis=1)
    gains, n = gl.check_conditions(name, env, what="%s x %d" % (shape, channels))
    gl.assert_bits(gains[:, -1], law.gain, "law_trace")
    print("%s %s x %d: %r" % (name, shape, channels, n))


@pytest.mark.parametrize("shape", list(gl.GLOBAL_RUNS))
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_rx_oracle_chain_global_gain(name, shape):
    """agc_global: the envelope of a block is the maximum over the channels (the loudest is at 100).  The conditions hold on that row."""
    channels = gl.GLOBAL_RUNS[shape]
    na, calls = unscaled(shape, channels, rows=1)
    spec = gl.rx_spec(shape, channels, rc.ARITH_CMSIS, gl.SETS[name], agc_global=True)
    orc, law = rc.CpuChain(spec, "orc"), nro.Agc(channels, na, gl.SETS[name], agc_global=True)
    for i, (iq, pre) in enumerate(calls):
        gl.assert_bits(orc.process(iq), law.process(pre), "%s %s call %d" % (name, shape, i))
    gains = orc.state()["agc_gain"]
    gl.assert_bits(gains, law.gain, "agc_gain")
    assert (gains == gains[0]).all()
    env = np.concatenate([gl.block_maxima(pre, na) for _, pre in calls], axis=1).max(axis=0, keepdims=True)
    gl.check_conditions(name, env, what="%s global" % shape)


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("shape", ["cfg3", "cfg2", "cfg4"])
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_rx_oracle_chain_global_gain_plain_plan(name, shape, q15):
    """agc_global on cfg3, cfg2 and cfg4 themselves, 130 channels, the six calls once: what tests/test_gpu_gain_law.py's other routes into the
    apply pass compare with (test_global_gain_other_routes, test_global_gain_in_two_phases).  One envelope row of 23 blocks: the oracle chain
    is pinned to the restatement on bits, and the row tells the set from the defaults; the other conditions stay with GLOBAL_RUNS."""
    channels = 130
    na, calls = unscaled(shape, channels, q15, plain=True)
    spec = gl.rx_spec(shape, channels, rc.ARITH_CMSIS, gl.SETS[name], agc_global=True)
    orc, law = rc.CpuChain(spec, "orc"), nro.Agc(channels, na, gl.SETS[name], agc_global=True)
    for i, (x, pre) in enumerate(calls):
        want = law.process(pre)
        gl.assert_bits(orc.process_q15(x) if q15 else orc.process(x), nro.float_to_q15(want) if q15 else want, "%s %s call %d" % (name, shape, i))
    gl.assert_bits(orc.state()["agc_gain"], law.gain, "agc_gain")
    env = np.concatenate([gl.block_maxima(pre, na) for _, pre in calls], axis=1).max(axis=0, keepdims=True)
    gl.check_defaults(name, env, what="%s global, plain plan" % shape)


@pytest.mark.parametrize("shape,channels", gl.Q15_RUNS)
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_rx_oracle_chain_int16_slots(name, shape, channels):
    """int16 slots (levels 10^-4 ... 1): orc_rx_process_q15 == arm_float_to_q15 of the restatement on the f32 audio of the converted input"""
    na, calls = unscaled(shape, channels, q15=True)
    spec = gl.rx_spec(shape, channels, rc.ARITH_CMSIS, gl.SETS[name])
    orc, law = rc.CpuChain(spec, "orc"), nro.Agc(channels, na, gl.SETS[name])
    for i, (q, pre) in enumerate(calls):
        gl.assert_bits(orc.process_q15(q), nro.float_to_q15(law.process(pre)), "%s %s call %d" % (name, shape, i))
    gl.assert_bits(orc.state()["agc_gain"], law.gain, "agc_gain")
    env = np.concatenate([gl.block_maxima(pre, na) for _, pre in calls], axis=1)
    if shape == "cfg4":      # (gain_law_cases.Q15_RUNS)
        gl.check_defaults(name, env, what="cfg4 int16")
    else:
        gl.check_conditions(name, env, what="%s int16" % shape)


# ---- 3. the TX oracle: the ALC sits in front of the chain, on the input audio ----------------------------------------------------------------
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("channels", gl.CHANNELS)
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_tx_oracle_equals_the_restatement(name, channels, q15):
    """TxCpuChain with alc_params == the same chain with its ALC off fed nr_oracle.Agc of the input audio (ALC blocks of 64 samples): I/Q of
    every call, alc_gain and every other row of the state, on bits"""
    on = rc.TxSpec(channels, alc_params=gl.SETS[name])
    a, b, law = rc.TxCpuChain(on, "orc"), rc.TxCpuChain(gl.no_gain(on), "orc"), nro.Agc(channels, on.block, gl.SETS[name])
    envs = []
    for i, x in enumerate(gl.plan(channels, on.block, gl.CALLS, q15, audio=True, **gl.run_kw("tx", channels, q15))):
        xf = gl.q15_to_f32(x) if q15 else x
        envs.append(gl.block_maxima(xf, on.block))
        want = b.process(law.process(xf))
        if q15:
            gl.assert_bits(a.process_q15(x), nro.float_to_q15(want), "%s call %d" % (name, i))
        else:
            gl.assert_bits(a.process(x), want, "%s call %d" % (name, i))
    sa, sb = a.state(), b.state()
    gl.assert_bits(sa["alc_gain"], law.gain, "alc_gain")
    for k in ("fir_state", "interp_state", "nco_phase"):
        gl.assert_bits(sa[k], sb[k], k)
    gl.check_conditions(name, np.concatenate(envs, axis=1), gl.TX_DEFAULTS, what="tx x %d" % channels)
