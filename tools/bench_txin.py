"""Time of the audio input stage of the TX chain (k_tx_in, csrc/tx_in.hip): C channels x B audio samples per call at the BASELINE-like
chain shape (DSP block 64, L = 4, 256-tap interpolator, 63-tap FIR pair), decimation by M with `taps` taps, VOX on with the gate, data
resident in HBM, everything in one process, each with its C-ABI timer (HIP events around `iters` launches or calls on the instance's stream).
Two variants, int16 stereo frames LEFT (the codec path, int16 audio out) and f32 stereo frames MIX (f32 audio out); for each:
  stage     the stage kernel alone (selenite_tx_time_in_stage_device)
  frames    the frame call: stage + chain (timed from the host around `iters` calls and a sync; the calls are asynchronous)
  audio     the f32 audio call of the same instance (selenite_tx_time_process_device); for the int16 variant also `audio_q15`, the int16
            audio entry the int16 frame call runs behind the stage, timed from the host as the frame call is
  copy      a device-to-device copy of the stage's read + written bytes (the yardstick of a streaming kernel)
The stage's bytes are given as a fraction of 8 TB/s and of the copy's rate.  Prints one JSON line; the variants alternate `rounds` times,
medians are reported.  `--isa` prints instead, for every instantiation of the kernel, the compiler's resource table and the counts of
the instruction kinds DESIGN section 5.18 speaks of (one JSON line each); it needs hipcc and no GPU."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selenite-lite_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--channels", type=int, default=16384)
ap.add_argument("--block-size", type=int, default=1024, help="audio samples per channel and call")
ap.add_argument("--decim", type=int, default=4)
ap.add_argument("--taps", type=int, default=64)
ap.add_argument("--arith", default="cmsis", choices=["fma", "cmsis"])
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--isa", action="store_true")
a = ap.parse_args()


def isa():
    pkg = os.path.join(ROOT, "selenite-lite_amd")
    flags = subprocess.run(["make", "-s", "-C", pkg, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    with tempfile.TemporaryDirectory() as tmp:
        s = os.path.join(tmp, "tx_in.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc"] + [f for f in flags if f != "--offload-compress"] +
                           ["--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", os.path.join(pkg, "csrc", "tx_in.hip"), "-o", s],
                           check=True, capture_output=True, text=True)
        text = open(s).read()
    res = {}
    for blk in r.stderr.split("Function Name: ")[1:]:
        name = blk.split()[0]
        res[name] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", blk)}
    kinds = ("v_fma_f32", "v_fmac_f32", "v_mad_f32", "v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32", "v_div_fmas_f32", "ds_read_b32", "ds_read2_b32",
             "ds_write_b32", "s_load_dwordx8", "s_load_dwordx4", "global_load_dwordx4", "global_store_dwordx4", "s_barrier", "scratch_")
    for body in re.split(r"\n(?=_Z\w+:[^\n]*\n)", text):
        m = re.match(r"(_Z\w+):", body)
        if not m or m.group(1) not in res:
            continue
        body = body.split(".Lfunc_end")[0]
        full = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout
        line = {"kernel": re.search(r"k_tx_in<[^>]*>", full).group(0)}
        line.update(res[m.group(1)])
        line.update({k: len(re.findall(r"\b" + k, body)) for k in kinds})
        print(json.dumps(line))


if a.isa:
    isa()
    raise SystemExit(0)

import numpy as np  # noqa: E402
import rxcommon as rc  # noqa: E402
import selenite_rx as sr  # noqa: E402

arith = {"fma": rc.ARITH_FMA, "cmsis": rc.ARITH_CMSIS}[a.arith]
C_, B, M = a.channels, a.block_size, a.decim
spec = rc.TxSpec(C_, arith=arith)
L = spec.interp
taps = sr.design_lowpass(a.taps, 0.4 / M)
vox = dict(gate=1, hang=4, attack=0.5, decay=0.125, open_level=1e-4, close_level=5e-5, level_init=0.0)
variants = {"q15_left": (sr.IN_Q15, sr.IN_LEFT, 2, 2), "f32_mix": (sr.IN_F32, sr.IN_MIX, 4, 4)}     # kind, pick, bytes per frame word, per audio sample

inst, d_fr, nbytes = {}, {}, {}
d_iq = sr.DeviceBuffer(C_ * B * L * 8)
rng = np.random.default_rng(rc.SEED)
for name, (kind, pick, wsz, asz) in variants.items():
    g = sr.Tx(spec.config())
    if g.set_in(M=M, coeffs=taps, pick=pick, gain=0.9, vox=vox):
        raise SystemExit("the library has no input stage")
    inst[name] = g
    words = B * M * 2
    d_fr[name] = sr.DeviceBuffer(C_ * words * wsz)
    chunk = 2048
    for c0 in range(0, C_, chunk):
        n = min(chunk, C_ - c0)
        x = rng.uniform(-0.5, 0.5, (n, words))
        x = x.astype(np.float32) if kind == sr.IN_F32 else np.round(x * 32768).astype(np.int16)
        sr.lib().selenite_rx_memcpy_h2d(d_fr[name].ptr + c0 * words * wsz, x.ctypes.data, x.nbytes)
    nbytes[name] = C_ * words * wsz + C_ * B * asz               # what the stage reads and writes
d_a = sr.DeviceBuffer(C_ * B * 4)
d_a.upload(np.zeros((C_, B), np.float32))
for c0 in range(0, C_, 4096):
    n = min(4096, C_ - c0)
    x = np.ascontiguousarray(sr.synth_iq_host(c0, n, 0, B, rc.SEED)[:, :, 0])
    sr.lib().selenite_rx_memcpy_h2d(d_a.ptr + c0 * B * 4, x.ctypes.data, x.nbytes)


def copy_ms(n, iters):
    """a device-to-device copy (hipMemcpyAsync) that moves the stage's bytes (n = read + written: n / 2 copied reads and writes as many):
    mean ms of `iters` copies between two HIP events, in this process (as tools/bench_out.py)"""
    import ctypes as C
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    vp = C.c_void_p
    hip.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    hip.hipEventCreate.argtypes = [C.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    hip.hipEventDestroy.argtypes = [vp]
    if n not in copy_bufs:
        copy_bufs[n] = (sr.DeviceBuffer(n // 2), sr.DeviceBuffer(n // 2))
    src, dst = copy_bufs[n]
    e0, e1 = vp(), vp()
    if hip.hipEventCreate(C.byref(e0)) or hip.hipEventCreate(C.byref(e1)):
        raise RuntimeError("hipEventCreate")
    hip.hipMemcpyAsync(dst.ptr, src.ptr, n // 2, 3, None)    # 3: hipMemcpyDeviceToDevice
    hip.hipEventRecord(e0, None)
    for _ in range(iters):
        if hip.hipMemcpyAsync(dst.ptr, src.ptr, n // 2, 3, None):
            raise RuntimeError("hipMemcpyAsync")
    hip.hipEventRecord(e1, None)
    hip.hipEventSynchronize(e1)
    t = C.c_float()
    hip.hipEventElapsedTime(C.byref(t), e0, e1)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    return t.value / iters


copy_bufs = {}


def frames_ms(name, iters):
    g, kind = inst[name], variants[name][0]
    assert g.sync() == 0
    t0 = time.perf_counter()
    for _ in range(iters):
        g.process_frames(d_fr[name].ptr, d_iq.ptr, B, kind)
    assert g.sync() == 0
    return (time.perf_counter() - t0) * 1e3 / iters


def audio_q15_ms(name, iters):
    """the int16 audio entry (selenite_tx_process_q15_device) on int16 audio, timed as frames_ms is: what the int16 frame call runs behind the stage"""
    g = inst[name]
    assert g.sync() == 0
    t0 = time.perf_counter()
    for _ in range(iters):
        g.L.selenite_tx_process_q15_device(g.h, d_a16.ptr, d_iq.ptr, B)
    assert g.sync() == 0
    return (time.perf_counter() - t0) * 1e3 / iters


d_a16 = sr.DeviceBuffer(C_ * B * 2)
d_a16.upload(np.zeros((C_, B), np.int16))
for c0 in range(0, C_, 4096):
    n = min(4096, C_ - c0)
    x = (np.ascontiguousarray(sr.synth_iq_host(c0, n, 0, B, rc.SEED)[:, :, 0]) * 32768.0).astype(np.int16)
    sr.lib().selenite_rx_memcpy_h2d(d_a16.ptr + c0 * B * 2, x.ctypes.data, x.nbytes)
runs = {"q15_left_audio_q15": lambda it: audio_q15_ms("q15_left", it)}
for name in variants:
    runs[name + "_stage"] = lambda it, n=name: inst[n].time_in_stage(d_fr[n].ptr, B, it, variants[n][0])
    runs[name + "_frames"] = lambda it, n=name: frames_ms(n, it)
    runs[name + "_audio"] = lambda it, n=name: inst[n].time_process(d_a.ptr, d_iq.ptr, B, it)
    runs[name + "_copy"] = lambda it, n=name: copy_ms(nbytes[n], it)
t0 = time.perf_counter()
while time.perf_counter() - t0 < 0.3:                      # steady-state clocks
    for f in runs.values():
        f(2)
t = {k: [] for k in runs}
for _ in range(a.rounds):
    for k, f in runs.items():
        t[k].append(f(a.iters))
med = {k: float(np.median(v)) for k, v in t.items()}
res = {"metric": "TX input stage: stage kernel alone, frame call, audio call, d2d copy of the stage's bytes; ms"}
res.update({k + "_ms": round(v, 4) for k, v in med.items()})
res.update({k + "_ms_runs": [round(x, 4) for x in v] for k, v in t.items()})
for name in variants:
    res[name + "_stage_bytes"] = nbytes[name]
    res[name + "_stage_fraction_of_8TBps"] = round(nbytes[name] / (med[name + "_stage"] * 1e-3) / 8e12, 4)
    res[name + "_stage_fraction_of_copy_rate"] = round(med[name + "_copy"] / med[name + "_stage"], 4)
res.update({"kernel_behind_the_stage": inst["f32_mix"].kernel_name(), "channels": C_, "audio_samples_per_call": B, "decim": M, "taps": a.taps,
            "interp": L, "arith": a.arith, "iters": a.iters, "rounds": a.rounds})
print(json.dumps(res))
