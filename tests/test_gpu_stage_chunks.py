"""GPU: the three stages (NLMS, output stage, spectrum tap) together on a host-pointer call that the pipeline cuts into ragged channel chunks,
and a refused split global-gain call on an instance with an output stage.  Every comparison is a bit comparison."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import rxcommon as rc
import selenite_rx as sr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_all_three_stages_across_ragged_channel_chunks(q15):
    """cfg3, 300 channels x 2048 samples with a 1 MiB chunk: 64-channel chunks for f32 slots (16 KiB of input per channel), 128-channel chunks
    for int16 slots, a ragged last chunk of 44 either way.  SELENITE_ARITH_AUTO with per-channel NCO steps: most pass bands are empty, so most
    channels of every chunk go through the rerun pass of a channel sub-range.  NLMS, the output stage (L = 4, stereo) and the spectrum tap
    (64 points, stride 1) are all on; over three streamed calls the host-pointer result equals the device-pointer result bit for bit: frames,
    chain state, NLMS state, interpolator state, spectrum rows, pending samples, position and frame count.  (A subprocess: the library reads
    SELENITE_RX_HOST_CHUNK_MB once.)"""
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import rxcommon as rc, selenite_rx as sr
        nch, bs, q15 = 300, 2048, %d
        steps = (np.arange(nch, dtype=np.uint64) * 0x9E3779B1 %% (1 << 32)).astype(np.uint32)
        spec = rc.baseline_spec("cfg3", nch, rc.ARITH_AUTO, nco_steps=steps)
        dev, hst = sr.Rx(spec.config()), sr.Rx(spec.config())
        h = sr.design_interp(32, 4, 0.1)
        for r in (dev, hst):
            r.set_nr(sr.NR_DENOISE, num_taps=16, delay=8, mu=0.05)
            r.set_out(4, h, sr.OUT_STEREO)
            r.set_spectrum(64, 1, 1, 0.25)
        dt = np.int16 if q15 else np.float32
        vals = dev.out_values(bs)
        assert vals == (bs // 4) * 4 * 2
        d_in, d_out = sr.DeviceBuffer(nch * bs * 2 * np.dtype(dt).itemsize), sr.DeviceBuffer(nch * vals * np.dtype(dt).itemsize)
        def same(a, b, what):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what
        for call in range(3):
            data = rc.synth_iq(0, nch, call * bs, bs)
            if q15:
                data = np.clip(np.trunc(data * 32768.0), -32768, 32767).astype(np.int16)
            d_in.upload(data)
            (dev.process_q15_device if q15 else dev.process_device)(d_in.ptr, d_out.ptr, bs)
            dev.sync()
            same((hst.process_q15 if q15 else hst.process)(data), d_out.download((nch, vals), dt), "frames of call %%d" %% call)
        for what, a, b in (("chain", dev.state(), hst.state()), ("nlms", dev.nr_state(), hst.nr_state()),
                           ("spectrum", dev.spectrum_state(), hst.spectrum_state())):
            assert sorted(a) == sorted(b), what
            for k in a:
                same(a[k], b[k], what + " state: " + k)
        same(dev.out_state(), hst.out_state(), "interpolator state")
        assert int(dev.spectrum_state()["position"][0]) == 3 * bs
        assert dev.spectrum()[1] == hst.spectrum()[1] == 3 * bs // 64
        rerun = dev.guard_stats()["rerun_channel_calls"]
        print("rerun channel-calls: %%d of %%d" %% (rerun, 3 * nch))
        assert 2 * rerun > 3 * nch and rerun == hst.guard_stats()["rerun_channel_calls"]      # "most channels": more than half of them
        print("OK")
    """ % (os.path.join(rc.ROOT, "tests"), rc.PKG_DIR, int(q15)))
    env = dict(os.environ, SELENITE_RX_HOST_CHUNK_MB="1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), (out.stdout[-1000:], out.stderr[-3000:])


def test_refused_split_global_gain_call_leaves_the_tap_alone():
    """The split global-gain calls exchange audio at the decimated rate, so an instance with an output stage refuses them with ARGUMENT_ERROR --
    before anything is launched: the spectrum tap's rows, pending samples, position and frame count are bit for bit what they were (the
    768-sample call before leaves the stream inside the second 512-point frame, so a tap that ran would move all four).  The refusal tested
    is the entry point's own (rx_api.hip), which comes before the dispatcher; the dispatcher's check in front of its tap hook
    (rx_dispatch.hip: run_chain) is an invariant behind it that no C-ABI call reaches, and this test does not guard its place."""
    ch, bs, n = 2, 768, 512
    rx = sr.Rx(rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS, agc_global=True).config())
    rx.set_out(4, sr.design_interp(32, 4, 0.1), sr.OUT_STEREO)
    rx.set_spectrum(n, 1, 1, 0.25)
    rx.process(rc.synth_iq(0, ch, 0, bs))
    before, frames = rx.spectrum_state(), rx.spectrum()[1]
    assert int(before["position"][0]) == bs and frames == 1 and np.any(before["rows"]) and np.any(before["pending"])
    d_in, d_out, d_env = sr.DeviceBuffer(ch * bs * 8), sr.DeviceBuffer(ch * (bs // 4) * 4), sr.DeviceBuffer(4 * (bs // 256))
    d_in.upload(rc.synth_iq(0, ch, bs, bs))
    rx.global_phase1(d_in.ptr, d_out.ptr, d_env.ptr, bs)
    assert rx.status() == sr.ARGUMENT_ERROR and "output stage" in rx.error()
    after = rx.spectrum_state()
    for k in ("rows", "pending", "position"):
        assert before[k].tobytes() == after[k].tobytes(), k
    assert rx.spectrum()[1] == frames
    d_in.free(); d_out.free(); d_env.free()
