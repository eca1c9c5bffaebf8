"""Time of the TX chain's FM mode (k_tx_fm, csrc/tx_fm.hip) beside the kernel it was modelled on: C channels x B audio samples per call at
the BASELINE-like shape (ALC block 64, L = 4, 256-tap interpolator, 63-tap FIR pair), data resident in HBM, both in one process, each with
selenite_tx_time_process_device (HIP events around `iters` calls on the instance's stream):
  (a) SELENITE_MODE_FM, tone on            -- k_tx_fm
  (b) SELENITE_MODE_USB, the same instance shape, SELENITE_RX_OPT_TX_FORCE_GENERIC -- k_tx_generic, which writes the same output bytes
The bar of the FM mode's issue is (a) <= 1.10 x (b).  Prints one JSON line; (a) and (b) alternate `rounds` times and the medians are reported."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selenite-lite_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import rxcommon as rc  # noqa: E402
import selenite_rx as sr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--channels", type=int, default=16384)
ap.add_argument("--block-size", type=int, default=1024, help="audio samples per channel and call")
ap.add_argument("--arith", default="cmsis", choices=["fma", "cmsis"])
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--no-tone", action="store_true")
a = ap.parse_args()
arith = {"fma": rc.ARITH_FMA, "cmsis": rc.ARITH_CMSIS}[a.arith]
steps = (np.arange(a.channels, dtype=np.uint64) * 0x00131313 + 0x00800000).astype(np.uint32)       # per-channel carriers: no shared LO for (b) either
spec = rc.TxSpec(a.channels, arith=arith, nco_steps=steps)
fm = sr.Tx(spec.config())
tsteps = np.array([sr.tone_step(hz, 48000.0) for hz in sr.ctcss_hz()], np.uint32)[np.arange(a.channels) % 50]
if fm.set_fm(0.25, 1.0, 0.1, None if a.no_tone else tsteps) or fm.set_mode(sr.MODE_FM):
    raise SystemExit("the library has no FM transmit mode")
with sr.plan_option(sr.OPT_TX_FORCE_GENERIC):
    gen = sr.Tx(spec.config())
assert fm.kernel_name() == "k_tx_fm" and gen.kernel_name() == "k_tx_generic"
L = spec.interp
d_a, d_iq = sr.DeviceBuffer(a.channels * a.block_size * 4), sr.DeviceBuffer(a.channels * a.block_size * L * 8)
chunk = 4096
for c0 in range(0, a.channels, chunk):
    n = min(chunk, a.channels - c0)
    x = np.ascontiguousarray(sr.synth_iq_host(c0, n, 0, a.block_size, rc.SEED)[:, :, 0])
    sr.lib().selenite_rx_memcpy_h2d(d_a.ptr + c0 * a.block_size * 4, x.ctypes.data, x.nbytes)
t0 = time.perf_counter()
while time.perf_counter() - t0 < 0.3:                      # steady-state clocks
    fm.time_process(d_a.ptr, d_iq.ptr, a.block_size, 2)
    gen.time_process(d_a.ptr, d_iq.ptr, a.block_size, 2)
t_fm, t_gen = [], []
for _ in range(a.rounds):
    t_fm.append(fm.time_process(d_a.ptr, d_iq.ptr, a.block_size, a.iters))
    t_gen.append(gen.time_process(d_a.ptr, d_iq.ptr, a.block_size, a.iters))
m_fm, m_gen = float(np.median(t_fm)), float(np.median(t_gen))
print(json.dumps({"metric": "TX FM call beside k_tx_generic (USB), ms per call", "fm_ms": round(m_fm, 4), "generic_usb_ms": round(m_gen, 4),
                  "ratio": round(m_fm / m_gen, 4), "bar": 1.10, "within_bar": bool(m_fm <= 1.10 * m_gen),
                  "fm_ms_runs": [round(v, 4) for v in t_fm], "generic_usb_ms_runs": [round(v, 4) for v in t_gen],
                  "fm_output_Msamples_per_s": round(a.channels * a.block_size * L / m_fm / 1e3, 1),
                  "channels": a.channels, "audio_samples_per_call": a.block_size, "interp": L, "arith": a.arith, "tone": not a.no_tone,
                  "iters": a.iters, "kernels": [fm.kernel_name(), gen.kernel_name()]}))
