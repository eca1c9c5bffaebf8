"""GPU: every restatement of the AGC / ALC gain law in the device code at non-default parameters (tests/gain_law_cases.py: the sets `odd`,
`fast`, `slow`; the level plan of six calls -- levels 1e-5 ... 100 over the channels, two calls 40 dB down, one silent).  No case here
passes the defaults; every case asserts its kernel_name().  tests/test_gain_law_oracle.py asserts on the CPU, from the restatement alone, that
these very runs meet the floor, both clamps and both branches and that a kernel with target * rcp(e), a fused update or a default carried as
a literal would differ in bits.

What is compared.  SELENITE_ARITH_CMSIS / _FMA, RX and TX: the audio (I/Q) of every call and the whole state behind the last one, on bits,
with the oracle chain of the same spec.  SELENITE_ARITH_SPLIT16 / _AUTO and TX split16: the law is exact arithmetic on whatever un-scaled
audio the kernel produced, so a twin of the same spec with its AGC off runs the same calls, and nr_oracle.Agc of the twin's audio must equal
the instance's audio and agc_gain on bits (every other row of the state: the twin's; AUTO: the same guard_stats()).  TX: the ALC sits in
front of the chain, so the twin (ALC off) is fed nr_oracle.Agc of the input audio and must give the same I/Q bits.  No tolerance anywhere.

The call sites (grep -n "agc_update\\|agc_desired\\|agc_step" selenite-lite_amd/csrc) and the cases that reach them:
  rx_device.h:199 agc_update, :213 agc_desired, :221 agc_step    the definitions: every case
  rx_fused_kernels.h:257 / :263  demod_agc_store<GROUP > 0>       test_rx_kernel_forms: cfg3, am, fm (16 lanes; cmsis on k_ssb_fused, fma on k_ssb_mfma),
                                                                  cfg2, cfg2_am, cfg3_1024 (64 lanes); the reruns and short calls of every auto case
  rx_fused_kernels.h:272         demod_agc_store<0> (run time)    test_rx_kernel_forms: fw96 (6 lanes, not a power of two), by8 (8), by2, cfg2_128 (32), cfg3_64 (4)
  rx_split16_kernels.h:98 / :105   agc_pass<16>                   test_rx_kernel_forms: cfg3 split16 / auto (k_ssb_split16)
  rx_split16_kernels.h:117 / :123  agc_pass<32>                   by2 split16 / auto (k_ssb_split16), cfg2_128 (k_hilb_split16)
  rx_split16_kernels.h:130         agc_pass<64>                   cfg3_1024 (k_ssb_split16), cfg2 and cfg2_am (k_hilb_split16; AM: its own branch)
  rx_split16_kernels.h:166 / :169  agc_pass<0> (run time)         fw96 (segmented scan), by8 (8 lanes: DPP), cfg3_64 (butterfly), am (whole rows)
  rx_cw.hip:406                  k_cw_fused                       test_rx_kernel_forms: cfg4
  rx_generic.hip:290             k_agc_generic                    test_rx_kernel_forms: wide, na14; test_generic_kernels_forced; test_stage_in_front_of_the_agc
                                                                  (the fused kernel with its AGC off, then this); test_int16_out_behind_the_iq_correction
  rx_generic.hip:403             k_agc_apply_global_rows          test_global_gain_apply_forms[cfg3_64]: na = 16 divides 256, calls of 1024 / 2048 (whole 256-output rows)
  rx_generic.hip:448             k_agc_apply_global, chunked      test_global_gain_apply_forms[cfg3_64]: the calls of 256 / 512 (64 / 128 outputs); int16 out: test_global_gain_other_routes[int16]
  rx_generic.hip:455             k_agc_apply_global, strided      test_global_gain_apply_forms[wide]: na = 512, 128 float4 per block
  rx_generic.hip:467             k_agc_apply_global, scalar       test_global_gain_apply_forms[na14]: na = 14
  tx_generic.hip:94              k_tx_generic                     test_tx_kernel_forms[generic]
  tx_fused.hip:143 / :147        k_tx_fused                       test_tx_kernel_forms[fused-cmsis / fused-fma], f32 and int16
  tx_fused.hip:408 / :412        k_tx_split16                     test_tx_kernel_forms[split16], f32 and int16
The seven parameters reach them through make_params (rx_dispatch.hip:75) / tx_api.hip:28, the initial gain through rx_api.hip:102 / tx_api.hip:94
(init and reset) and, for a host-pointer call cut into channel chunks, through the chunk's channel range: test_host_call_in_ragged_channel_chunks,
test_reset_returns_to_the_configured_gain.

int16 out (test_int16_slots, the q15 cases): a one-ulp change of the gain shows in int16 audio only where it moves a sample across an integer,
so those cases pin the parameters and the initial gain in the int16 instantiations; the f32 cases of the same kernels pin the last bit
(gain_law_cases.Q15_RUNS).  The reset tests replay a stream against itself: they pin gain_init, not the arithmetic.

A run of under 16 envelope rows (3 channels; a global gain: ONE row) repeats the six calls until it has 2400 envelopes, with a level walk on
top, and a few runs need more than that (gain_law_cases.plan, RUNS); FM takes the plan's levels as its deviation.  The CPU test asserts every
condition for all three sets on every run of test_rx_kernel_forms, test_global_gain_apply_forms and test_tx_kernel_forms."""
import functools
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import gain_law_cases as gl
import nr_oracle as nro
import rxcommon as rc
import selenite_rx as sr

pytestmark = pytest.mark.gpu
EXACT = (rc.ARITH_CMSIS, rc.ARITH_FMA)
f32 = np.float32


def assert_state(got, want, what, skip=()):
    assert set(got) == set(want)
    for k in want:
        if k not in skip:
            gl.assert_bits(got[k], want[k], "%s: state %s" % (what, k))


def run_device(rx, data):
    q15 = data.dtype == np.int16
    ch, bs = data.shape[0], data.shape[1]
    vals = rx.out_len(bs)
    d_in, d_out = sr.DeviceBuffer(data.nbytes), sr.DeviceBuffer(ch * vals * data.dtype.itemsize)
    d_in.upload(np.ascontiguousarray(data))
    (rx.process_q15_device if q15 else rx.process_device)(d_in.ptr, d_out.ptr, bs)
    rx.sync()
    rx.check()
    out = d_out.download((ch, vals), data.dtype)
    d_in.free(); d_out.free()
    return out


def run(rx, data, device=False):
    if device:
        return run_device(rx, data)
    return rx.process_q15(data) if data.dtype == np.int16 else rx.process(data)


@functools.lru_cache(maxsize=4)
def rx_plan(shape, channels, q15=False, rows=None, plain=False):
    return gl.rx_plan(shape, channels, q15, rows, plain)


@functools.lru_cache(maxsize=4)
def tx_plan(channels, q15=False):
    return gl.plan(channels, 64, gl.CALLS, q15, audio=True, **gl.run_kw("tx", channels, q15))


def make_rx(spec, generic=False, prepare=None):
    if generic:
        with sr.plan_option(sr.OPT_FORCE_GENERIC):
            rx = sr.Rx(spec.config())
    else:
        rx = sr.Rx(spec.config())
    if prepare:
        prepare(rx)
    return rx


def stream_rx(spec, name, kernel, calls, generic=False, prepare=None, twin=None):
    """One instance of `spec` (set `name`) over the calls of the plan, host- and device-pointer calls in turn, against the oracle chain
    (_CMSIS / _FMA) or against nr_oracle.Agc of a twin's un-scaled audio (twin: _SPLIT16 / _AUTO, and where asked)."""
    ch, na, q15 = spec.channels, spec.block // spec.decim, calls[0].dtype == np.int16
    assert spec.agc and spec.agc_params["gain_init"] == gl.SETS[name]["gain_init"] != 1.0
    a = make_rx(spec, generic, prepare)
    assert a.kernel_name() == kernel, a.kernel_name()
    twin = spec.arith not in EXACT if twin is None else twin
    if twin:
        b, law = make_rx(gl.no_gain(spec), generic, prepare), nro.Agc(ch, na, gl.SETS[name], agc_global=spec.agc_global)
        assert b.kernel_name() == kernel, b.kernel_name()
    else:
        orc = rc.CpuChain(spec, "orc")
        assert orc.ok()
    for i, x in enumerate(calls):
        what = "%s %s x %d call %d (%d)" % (name, kernel, ch, i, x.shape[1])
        got = run(a, x, device=i % 2 == 1)
        if twin:
            want = law.process(run(b, gl.q15_to_f32(x) if q15 else x, device=i % 2 == 1))
            want = nro.float_to_q15(want, spec.q15_rounding) if q15 else want
        else:
            want = orc.process_q15(x) if q15 else orc.process(x)
        gl.assert_bits(got, want, what)
    if twin:
        gl.assert_bits(a.state()["agc_gain"], law.gain, "%s %s: agc_gain" % (name, kernel))
        assert_state(a.state(), b.state(), name + " " + kernel, skip=("agc_gain",))
        if spec.arith == rc.ARITH_AUTO:
            assert a.guard_stats() == b.guard_stats()
        b.close()
    else:
        assert_state(a.state(), orc.state(), name + " " + kernel)
    a.close()


def form_id(v):
    return gl.ARITH_NAME.get(v, v) if isinstance(v, int) else v


# ---- 1. one instance per kernel form -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", gl.CHANNELS)
@pytest.mark.parametrize("name,shape,arith", gl.RX_FORMS, ids=["%s-%s-%s" % (n, s, gl.ARITH_NAME[a]) for n, s, a in gl.RX_FORMS])
def test_rx_kernel_forms(name, shape, arith, channels):
    """gain_law_cases.RX_SHAPES says which group size and which kernel every shape selects; the module docstring maps them to the call sites"""
    spec = gl.rx_spec(shape, channels, arith, gl.SETS[name])
    stream_rx(spec, name, gl.rx_kernel(shape, arith), rx_plan(shape, channels))


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("arith", EXACT, ids=["cmsis", "fma"])
@pytest.mark.parametrize("shape", ["cfg3", "cfg4"])
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_generic_kernels_forced(name, shape, arith, q15):
    """sr.plan_option(sr.OPT_FORCE_GENERIC): k_front_generic (+ k_biquad_generic) and k_agc_generic<ARITH, float / int16_t> serve the call"""
    spec = gl.rx_spec(shape, 65, arith, gl.SETS[name])
    stream_rx(spec, name, "generic", rx_plan(shape, 65, q15), generic=True)


# ---- 2. the global gain -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", EXACT, ids=["cmsis", "fma"])
@pytest.mark.parametrize("shape", list(gl.GLOBAL_RUNS))
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_global_gain_apply_forms(name, shape, arith):
    """agc_global in one call: gain_law_cases.GLOBAL_RUNS says which of the four forms of the apply pass (rx_generic.hip:
    launch_agc_apply_global) each shape and call length selects.  One envelope row: the sparse plan."""
    spec = gl.rx_spec(shape, gl.GLOBAL_RUNS[shape], arith, gl.SETS[name], agc_global=True)
    stream_rx(spec, name, gl.rx_kernel(shape, arith), rx_plan(shape, spec.channels, rows=1))


ROUTES = {
    # k_ssb_split16 leaves the block maxima of every channel behind (env_part) on the calls of 1024 / 2048 samples (whole passes) and does
    # not on those of 256 / 512: launch_env_fold over channels x blocks floats there, k_env_global over the audio here
    "split16-env_part": ("cfg3", rc.ARITH_SPLIT16, {}),
    "auto": ("cfg3", rc.ARITH_AUTO, {}),
    "hilb-split16": ("cfg2", rc.ARITH_SPLIT16, {}),
    "cw": ("cfg4", rc.ARITH_CMSIS, {}),
    "int16": ("cfg3", rc.ARITH_CMSIS, dict(q15=True)),                 # k_agc_apply_global<ARITH, int16_t>, chunked form, every call
    "forced-generic": ("cfg3", rc.ARITH_FMA, dict(generic=True)),
}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_global_gain_other_routes(name, route):
    """Other ways into the same apply pass, the plain six calls on 130 channels: what differs is who leaves the un-scaled audio and the
    envelope row (the conditions for the pass itself are test_global_gain_apply_forms'; tests/test_gain_law_oracle.py pins the oracle chain of
    these runs to the restatement and tells their envelope row from the defaults: test_rx_oracle_chain_global_gain_plain_plan)."""
    shape, arith, kw = ROUTES[route]
    spec = gl.rx_spec(shape, 130, arith, gl.SETS[name], agc_global=True)
    generic = kw.get("generic", False)
    stream_rx(spec, name, "generic" if generic else gl.rx_kernel(shape, arith), rx_plan(shape, 130, kw.get("q15", False), plain=True), generic=generic)


@pytest.mark.parametrize("arith", [rc.ARITH_CMSIS, rc.ARITH_SPLIT16], ids=["cmsis", "split16"])
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_global_gain_in_two_phases(name, arith):
    """global_phase1 + global_phase2 on cfg3, 130 channels: phase 1 leaves the un-scaled audio and the envelope row (bits of the block maxima
    over the channels; split16: from env_part on whole passes), phase 2 the law on that row: nr_oracle.Agc of phase 1's audio, and in _CMSIS
    the oracle chain"""
    ch = 130
    spec = gl.rx_spec("cfg3", ch, arith, gl.SETS[name], agc_global=True)
    rx, law = sr.Rx(spec.config()), nro.Agc(ch, 64, gl.SETS[name], agc_global=True)
    assert rx.kernel_name() == gl.rx_kernel("cfg3", arith)
    orc = rc.CpuChain(spec, "orc") if arith in EXACT else None
    for i, iq in enumerate(rx_plan("cfg3", ch, plain=True)):
        bs = iq.shape[1]
        nblk = bs // 256
        d_in, d_out, d_env = sr.DeviceBuffer(iq.nbytes), sr.DeviceBuffer(ch * (bs // 4) * 4), sr.DeviceBuffer(nblk * 4)
        d_in.upload(iq)
        rx.global_phase1(d_in.ptr, d_out.ptr, d_env.ptr, bs)
        rx.sync(); rx.check()
        pre, env = d_out.download((ch, bs // 4), f32), d_env.download((nblk,), f32)
        gl.assert_bits(env, gl.block_maxima(pre, 64).max(axis=0), "call %d: envelope row" % i)
        rx.global_phase2(d_out.ptr, d_env.ptr, bs)
        rx.sync(); rx.check()
        got = d_out.download((ch, bs // 4), f32)
        gl.assert_bits(got, law.process(pre, env=env), "%s call %d" % (name, i))
        if orc:
            gl.assert_bits(got, orc.process(iq), "%s call %d: oracle chain" % (name, i))
        d_in.free(); d_out.free(); d_env.free()
    gl.assert_bits(rx.state()["agc_gain"], law.gain, "agc_gain")
    if orc:
        assert_state(rx.state(), orc.state(), name)


# ---- 3. the law behind another stage, and the slot formats ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,arith", [("cfg3", rc.ARITH_CMSIS), ("cfg3", rc.ARITH_AUTO), ("cfg2", rc.ARITH_SPLIT16), ("cfg4", rc.ARITH_FMA)], ids=form_id)
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_stage_in_front_of_the_agc(name, q15, shape, arith):
    """The level meter with gate = 0 (a tap: it changes no audio): the fused kernel runs with its own AGC off and k_agc_generic finishes the
    call, f32 and int16 out"""
    spec = gl.rx_spec(shape, 65, arith, gl.SETS[name])
    stream_rx(spec, name, gl.rx_kernel(shape, arith), rx_plan(shape, 65, q15), prepare=lambda r: r.set_meter(gate=0))


@pytest.mark.parametrize("shape,arith", [("cfg3", rc.ARITH_CMSIS), ("cfg3", rc.ARITH_SPLIT16), ("cfg3", rc.ARITH_AUTO), ("cfg2", rc.ARITH_CMSIS),
                                         ("cfg2", rc.ARITH_AUTO), ("cfg2_128", rc.ARITH_SPLIT16), ("cfg4", rc.ARITH_CMSIS), ("fw96", rc.ARITH_CMSIS)], ids=form_id)
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_int16_slots(name, shape, arith):
    """int16 slots in and out (levels 1e-4 ... 1): the law inside the int16 instantiations of the fused kernels; 130 channels"""
    spec = gl.rx_spec(shape, 130, arith, gl.SETS[name])
    stream_rx(spec, name, gl.rx_kernel(shape, arith), rx_plan(shape, 130, True))


@pytest.mark.parametrize("arith", [rc.ARITH_CMSIS, rc.ARITH_AUTO], ids=["cmsis", "auto"])
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_int16_out_behind_the_iq_correction(name, arith):
    """int16 slots with the I/Q correction on: the stage's copy is f32, so the call runs f32 in, int16 out (`mixed`, rx_dispatch.hip: run_part)
    -- the fused kernel with its AGC off into the f32 scratch, k_agc_generic<ARITH, int16_t> behind it.  The twin (AGC off, the same
    correction, f32 slots of the converted input) gives the un-scaled audio in every arith mode."""
    spec = gl.rx_spec("cfg3", 65, arith, gl.SETS[name])
    stream_rx(spec, name, gl.rx_kernel("cfg3", arith), rx_plan("cfg3", 65, True), prepare=lambda r: r.set_iqc(frame=64), twin=True)


# ---- 4. the initial gain: reset, the state round trip, channel chunks of a host-pointer call -------------------------------------------------------
RESETS = {"cfg3-cmsis": ("cfg3", rc.ARITH_CMSIS, {}), "cfg3-split16": ("cfg3", rc.ARITH_SPLIT16, {}), "cfg2-auto": ("cfg2", rc.ARITH_AUTO, {}),
          "cfg4-fma": ("cfg4", rc.ARITH_FMA, {}), "na14-generic": ("na14", rc.ARITH_CMSIS, {}), "cfg3-global": ("cfg3", rc.ARITH_CMSIS, dict(agc_global=True))}


@pytest.mark.parametrize("kind", list(RESETS))
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_reset_returns_to_the_configured_gain(name, kind):
    """reset() in the middle of a stream: agc_gain is gain_init again (2.3, 0.25, 7.5 -- not 1), and the stream's first calls replayed give
    the bits they gave (the kernel_forms cases compare those with the oracle).  Then state() / set_state(): a gain row of the caller's is
    read back as bits and is where the next call starts (nr_oracle.Agc of the AGC-off twin's audio from those gains)."""
    shape, arith, kw = RESETS[kind]
    ch, p = 65, gl.SETS[name]
    spec = gl.rx_spec(shape, ch, arith, p, **kw)
    rx, twin = sr.Rx(spec.config()), sr.Rx(gl.no_gain(spec).config())
    assert rx.kernel_name() == gl.rx_kernel(shape, arith)
    calls = rx_plan(shape, ch, plain=True)
    init = np.full(ch, p["gain_init"], f32)
    gl.assert_bits(rx.state()["agc_gain"], init, "agc_gain of a new instance")
    first = [rx.process(x) for x in calls[:3]]
    assert not (rx.state()["agc_gain"] == init).any()
    assert rx.reset() == 0
    gl.assert_bits(rx.state()["agc_gain"], init, "agc_gain behind reset()")
    for i, x in enumerate(calls[:3]):
        gl.assert_bits(rx.process(x), first[i], "%s %s: call %d replayed behind reset()" % (name, kind, i))
        twin.process(x)
    st = rx.state()
    st["agc_gain"] = (f32(p["gain_min"]) + (f32(p["gain_max"]) - f32(p["gain_min"])) * np.linspace(0, 1, ch) ** 3).astype(f32)
    rx.set_state(st)
    assert_state(rx.state(), st, "set_state() / state()")
    law = nro.Agc(ch, spec.block // spec.decim, p, agc_global=spec.agc_global)
    law.gain = st["agc_gain"].copy()
    gl.assert_bits(rx.process(calls[3]), law.process(twin.process(calls[3])), "%s %s: the call behind set_state()" % (name, kind))
    gl.assert_bits(rx.state()["agc_gain"], law.gain, "agc_gain")


def test_host_call_in_ragged_channel_chunks():
    """cfg3, 300 channels x 2048 samples through the host-pointer entry with a 1 MiB chunk: channel chunks of 64 and a ragged last one of 44.
    Every chunk's channels start from the configured gain (`odd`: 2.3; then `fast` and `slow`) and carry their own gain into the second call:
    audio and state equal the oracle chain's on bits.  (A subprocess: the library reads SELENITE_RX_HOST_CHUNK_MB once.)"""
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import gain_law_cases as gl, rxcommon as rc, selenite_rx as sr
        nch, bs = 300, 2048
        lv = gl.levels(nch)[:, None, None]
        for name in gl.SET_NAMES:
            spec = gl.rx_spec("cfg3", nch, rc.ARITH_CMSIS, gl.SETS[name])
            rx, orc = sr.Rx(spec.config()), rc.CpuChain(spec, "orc")
            assert rx.kernel_name() == gl.rx_kernel("cfg3", rc.ARITH_CMSIS)
            for call in range(2):
                iq = np.ascontiguousarray(rc.synth_iq(0, nch, call * bs, bs) * lv * np.float32(0.01 if call else 1.0), np.float32)
                got, want = rx.process(iq), orc.process(iq)
                assert got.tobytes() == want.tobytes(), (name, call, np.argwhere(got != want)[:4])
            sg, so = rx.state(), orc.state()
            for k in so:
                assert sg[k].tobytes() == so[k].tobytes(), (name, k)
            assert not (sg["agc_gain"] == np.float32(gl.SETS[name]["gain_init"])).any()
        print("OK")
    """ % (os.path.join(rc.ROOT, "tests"), rc.PKG_DIR))
    env = dict(os.environ, SELENITE_RX_HOST_CHUNK_MB="1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), (out.stdout[-1000:], out.stderr[-3000:])


# ---- 5. TX: the ALC ---------------------------------------------------------------------------------------------------------------------------------
TX_FORMS = {"generic": (rc.ARITH_CMSIS, True, "k_tx_generic"), "fused-cmsis": (rc.ARITH_CMSIS, False, "k_tx_fused<4,256,63>"),
            "fused-fma": (rc.ARITH_FMA, False, "k_tx_fused<4,256,63>"), "split16": (rc.ARITH_SPLIT16, False, "k_tx_split16<4,256,63>")}


def make_tx(spec, generic):
    if generic:
        with sr.plan_option(sr.OPT_TX_FORCE_GENERIC):
            return sr.Tx(spec.config())
    return sr.Tx(spec.config())


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("channels", gl.CHANNELS)
@pytest.mark.parametrize("form", list(TX_FORMS))
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_tx_kernel_forms(name, form, channels, q15):
    """TxSpec(alc_params=...), ALC blocks of 64 samples, the six calls of the plan on the TX input.  Exact arithmetic: the TX oracle on bits.
    k_tx_split16: alc_gain equals nr_oracle.Agc of the input audio, and the I/Q equals the I/Q of a twin with its ALC off that is fed the
    restatement's scaled audio (the same kernel on the same numbers)."""
    arith, generic, kernel = TX_FORMS[form]
    spec = rc.TxSpec(channels, arith=arith, alc_params=gl.SETS[name])
    a = make_tx(spec, generic)
    assert a.kernel_name() == kernel, a.kernel_name()
    twin = arith not in EXACT
    if twin:
        b, law = make_tx(gl.no_gain(spec), generic), nro.Agc(channels, spec.block, gl.SETS[name])
    else:
        orc = rc.TxCpuChain(spec, "orc")
    for i, x in enumerate(tx_plan(channels, q15)):
        got = a.process_q15(x) if q15 else a.process(x)
        if twin:
            want = b.process(law.process(gl.q15_to_f32(x) if q15 else x))
            want = nro.float_to_q15(want) if q15 else want
        else:
            want = orc.process_q15(x) if q15 else orc.process(x)
        gl.assert_bits(got, want, "%s %s x %d call %d" % (name, kernel, channels, i))
    if twin:
        gl.assert_bits(a.state()["alc_gain"], law.gain, "alc_gain")
        assert_state(a.state(), b.state(), name + " " + kernel, skip=("alc_gain",))
        b.close()
    else:
        assert_state(a.state(), orc.state(), name + " " + kernel)
    a.close()


@pytest.mark.parametrize("form", list(TX_FORMS))
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_tx_reset_returns_to_the_configured_gain(name, form):
    arith, generic, kernel = TX_FORMS[form]
    ch, p = 65, gl.SETS[name]
    tx = make_tx(rc.TxSpec(ch, arith=arith, alc_params=p), generic)
    assert tx.kernel_name() == kernel
    calls = tx_plan(ch)
    init = np.full(ch, p["gain_init"], f32)
    gl.assert_bits(tx.state()["alc_gain"], init, "alc_gain of a new instance")
    first = [tx.process(x) for x in calls[:3]]
    assert not (tx.state()["alc_gain"] == init).any()
    assert tx.reset() == 0
    gl.assert_bits(tx.state()["alc_gain"], init, "alc_gain behind reset()")
    for i, x in enumerate(calls[:3]):
        gl.assert_bits(tx.process(x), first[i], "%s %s: call %d replayed behind reset()" % (name, kernel, i))
    tx.close()
