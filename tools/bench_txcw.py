"""Time of the keyed CW path of the TX chain (k_tx_cw, csrc/tx_cw.hip) beside the kernels it was modelled on: C channels x B audio samples
per call at the BASELINE-like shape (DSP block 64, L = 4, 256-tap interpolator, 63-tap FIR pair, per-channel carriers), a 64-tap Hann
keying shape, data resident in HBM, everything in one process, each with its C-ABI timer (HIP events around `iters` calls on the instance's
stream):
  keyed, sidetone off / on, 50 %-duty random keying (elements of 128 to 511 samples) / key held        -- k_tx_cw
  SELENITE_MODE_FM, tone off, the same instance shape                                                  -- k_tx_fm (the yardstick)
  SELENITE_MODE_USB, the same instance shape, SELENITE_RX_OPT_TX_FORCE_GENERIC                          -- k_tx_generic
The bar of the keyed path's issue: the keyed call with the sidetone off takes no longer than k_tx_fm.  All write the same I/Q bytes; the
store bandwidth is given as a fraction of 8 TB/s.  Prints one JSON line; the variants alternate `rounds` times, medians are reported."""
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
ap.add_argument("--shape-taps", type=int, default=64)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
arith = {"fma": rc.ARITH_FMA, "cmsis": rc.ARITH_CMSIS}[a.arith]
C_, B = a.channels, a.block_size
steps = (np.arange(C_, dtype=np.uint64) * 0x00131313 + 0x00800000).astype(np.uint32)       # per-channel carriers, as tools/bench_txfm.py
spec = rc.TxSpec(C_, arith=arith, nco_steps=steps, mode=rc.MODE_CW)
L = spec.interp
cw = sr.Tx(spec.config())
if cw.set_cw(sr.keyshape(a.shape_taps), 0.9, sr.tone_step(700.0, 12000.0 * L), 0.25, sr.tone_step(700.0, 12000.0), 0, 5):
    raise SystemExit("the library has no keyed CW path")
fm = sr.Tx(spec.config())
assert fm.set_fm(0.25, 1.0, 0.0, None) == 0 and fm.set_mode(sr.MODE_FM) == 0
with sr.plan_option(sr.OPT_TX_FORCE_GENERIC):
    gen = sr.Tx(spec.config())
assert gen.set_mode(rc.MODE_USB) == 0
assert fm.kernel_name() == "k_tx_fm" and gen.kernel_name() == "k_tx_generic"

rng = np.random.default_rng(rc.SEED)
keys = np.zeros((C_, B), np.uint8)
for c in range(C_):                                        # random elements and gaps of 128 to 511 samples: half the time down
    at, v = -int(rng.integers(0, 512)), int(rng.integers(0, 2))
    while at < B:
        ln = int(rng.integers(128, 512))
        keys[c, max(at, 0):max(at + ln, 0)] = v
        at, v = at + ln, 1 - v
d_rand, d_held = sr.DeviceBuffer(C_ * B), sr.DeviceBuffer(C_ * B)
d_rand.upload(keys)
d_held.upload(np.ones((C_, B), np.uint8))
d_a, d_iq, d_side = sr.DeviceBuffer(C_ * B * 4), sr.DeviceBuffer(C_ * B * L * 8), sr.DeviceBuffer(C_ * B * 4)
chunk = 4096
for c0 in range(0, C_, chunk):
    n = min(chunk, C_ - c0)
    x = np.ascontiguousarray(sr.synth_iq_host(c0, n, 0, B, rc.SEED)[:, :, 0])
    sr.lib().selenite_rx_memcpy_h2d(d_a.ptr + c0 * B * 4, x.ctypes.data, x.nbytes)
d_side.upload(np.zeros((C_, B), np.float32))

runs = {
    "keyed_random": lambda it: cw.time_process_key(d_rand.ptr, d_iq.ptr, None, B, it),
    "keyed_held": lambda it: cw.time_process_key(d_held.ptr, d_iq.ptr, None, B, it),
    "keyed_random_sidetone": lambda it: cw.time_process_key(d_rand.ptr, d_iq.ptr, d_side.ptr, B, it),
    "keyed_held_sidetone": lambda it: cw.time_process_key(d_held.ptr, d_iq.ptr, d_side.ptr, B, it),
    "fm": lambda it: fm.time_process(d_a.ptr, d_iq.ptr, B, it),
    "generic_usb": lambda it: gen.time_process(d_a.ptr, d_iq.ptr, B, it),
}
t0 = time.perf_counter()
while time.perf_counter() - t0 < 0.3:                      # steady-state clocks
    for f in runs.values():
        f(2)
t = {k: [] for k in runs}
for _ in range(a.rounds):
    for k, f in runs.items():
        t[k].append(f(a.iters))
med = {k: float(np.median(v)) for k, v in t.items()}
out_bytes = C_ * B * L * 8
res = {"metric": "keyed CW call beside k_tx_fm (tone off) and k_tx_generic (USB), ms per call"}
res.update({k + "_ms": round(v, 4) for k, v in med.items()})
res.update({k + "_ms_runs": [round(x, 4) for x in v] for k, v in t.items()})
res.update({k + "_store_fraction_of_8TBps": round(out_bytes / (med[k] * 1e-3) / 8e12, 4) for k in runs})
res.update({"ratio_random_to_fm": round(med["keyed_random"] / med["fm"], 4), "ratio_held_to_fm": round(med["keyed_held"] / med["fm"], 4),
            "bar": "keyed (sidetone off) <= fm", "within_bar": bool(med["keyed_random"] <= med["fm"] and med["keyed_held"] <= med["fm"]),
            "key_duty": round(float(keys.mean()), 4), "channels": C_, "audio_samples_per_call": B, "interp": L, "shape_taps": a.shape_taps,
            "arith": a.arith, "iters": a.iters, "rounds": a.rounds, "timed_calls_per_variant": a.iters * a.rounds})
print(json.dumps(res))
