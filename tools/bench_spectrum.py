#!/usr/bin/env python3
"""tools/bench_spectrum.py -- what the spectrum tap (selenite_rx_set_spectrum) costs at full size: cfg3 (65 536 channels x 4096 samples, _AUTO)
and cfg2 (4096 channels x 48 000 samples), f32 and int16 slots, with the tap off and with N = 512 at stride 1 and 8 and N = 64 at stride 1
(averaging on, Hann window): ms per call (median of --iters launches, one HIP event between calls, as bench.py takes them), the tap's added
ms, the bytes the tap kernel moves (the frames it reads; the row in and out), and a device-to-device copy of the same number of bytes timed
in the same process (hipMemcpyAsync of (read + written) / 2 bytes: it reads and writes that many).
--only off: the tap-off rows alone (for an A/B against another build named by SELENITE_RX_LIB); --only tap: the cfg3 f32 rows alone (a short
run for a kernel trace).
--isa: no GPU; compiles csrc/rx_spectrum.hip for gfx950 with the library's flags and reads, per k_spectrum<N, TIn>, the VGPR use, the vector
and LDS instructions (static counts; the frame loop is straight-line code), the barriers, and whether any fused multiply-add sits in the kernel.
One JSON line per row."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selenite-lite_amd"))
import numpy as np  # noqa: E402
import selenite_rx as sr  # noqa: E402
from selenite_rx import chain as ch  # noqa: E402

CONFIGS = {"cfg3": ("cfg3", 65536, 4096), "cfg2": ("cfg2_48k128", 4096, 48000)}
TAPS = [(512, 1), (512, 8), (64, 1)]


def time_call(cfg, iters, q15, tap):
    """median ms per call in _AUTO; tap: None or (fft_len, stride)"""
    name, channels, nsamp = CONFIGS[cfg]
    spec = ch.baseline_spec(name, channels, sr.ARITH_AUTO)
    rx = sr.Rx(spec.config())
    if tap is not None:
        rx.set_spectrum(tap[0], tap[1], 1, 0.25, sr.design_window(tap[0], sr.WINDOW_HANN))
    esz = 2 if q15 else 4
    d_in, d_out = sr.DeviceBuffer(channels * nsamp * 2 * esz), sr.DeviceBuffer(channels * (nsamp // spec.decim) * esz)
    if q15:
        f = sr.DeviceBuffer(channels * nsamp * 8)
        rx.synth_device(f.ptr, 0, channels, 0, nsamp, ch.SEED)
        rx.sync()
        host = f.download((channels, nsamp, 2), np.float32)
        d_in.upload((host * 32768.0).astype(np.int16))
        f.free()
    else:
        rx.synth_device(d_in.ptr, 0, channels, 0, nsamp, ch.SEED)
    rx.time_process_each(d_in.ptr, d_out.ptr, nsamp, 3, q15)
    ms = rx.time_process_each(d_in.ptr, d_out.ptr, nsamp, iters, q15)
    rx.sync()
    rx.close()
    d_in.free(); d_out.free()
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def copy_ms(nbytes, iters):
    """a device-to-device copy (hipMemcpyAsync) that moves `nbytes` in all (half read, half written): median ms of `iters` copies, one HIP
    event between copies, in this process"""
    import ctypes as C
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    vp = C.c_void_p
    hip.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    hip.hipEventCreate.argtypes = [C.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    hip.hipEventDestroy.argtypes = [vp]
    n = nbytes // 2
    a, b = sr.DeviceBuffer(n), sr.DeviceBuffer(n)
    ev = [vp() for _ in range(iters + 1)]
    for e in ev:
        if hip.hipEventCreate(C.byref(e)):
            raise RuntimeError("hipEventCreate")
    d2d = 3                                                  # hipMemcpyDeviceToDevice
    for _ in range(3):
        hip.hipMemcpyAsync(b.ptr, a.ptr, n, d2d, None)
    hip.hipEventRecord(ev[0], None)
    for i in range(iters):
        if hip.hipMemcpyAsync(b.ptr, a.ptr, n, d2d, None):
            raise RuntimeError("hipMemcpyAsync")
        hip.hipEventRecord(ev[i + 1], None)
    hip.hipEventSynchronize(ev[iters])
    ms = []
    for i in range(iters):
        t = C.c_float()
        hip.hipEventElapsedTime(C.byref(t), ev[i], ev[i + 1])
        ms.append(t.value)
    for e in ev:
        hip.hipEventDestroy(e)
    a.free(); b.free()
    return float(np.median(ms))


def tap_bytes(cfg, q15, tap):
    """what one call of the tap kernel moves once the stream runs: the transformed frames' samples, the row in and out (pending: the part of
    a frame a call ends in, in and out, where the call is no whole number of frames -- cfg2's 48 000 = 93.75 frames of 512)"""
    _, channels, nsamp = CONFIGS[cfg]
    n, stride = tap
    frames = nsamp / n / stride
    rd = channels * (frames * n * (4 if q15 else 8) + n * 4)
    wr = channels * n * 4
    if nsamp % n:
        rd += channels * (nsamp % n) * 8 / stride
        wr += channels * (nsamp % n) * 8 / stride
    return int(rd), int(wr)


def isa_rows():
    pkg = os.path.join(ROOT, "selenite-lite_amd")
    flags = subprocess.run(["make", "-s", "-C", pkg, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    flags = [f for f in flags if f != "--offload-compress"] + os.environ.get("BENCH_SPECTRUM_EXTRA_FLAGS", "").split()
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "rx_spectrum.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", "-o", asm,
                        os.path.join(pkg, "csrc", "rx_spectrum.hip")], check=True, capture_output=True)
        text = open(asm).read()
    kern, cur, blk = {}, None, None
    for line in text.split("\n"):
        t = line.split(";")[0].strip()
        m = re.match(r"^_ZN3srx10k_spectrumILi(\d+)E([fs])E\S*:$", t)
        if m:
            cur = (int(m.group(1)), m.group(2)); blk = []; kern[cur] = {"blocks": [blk], "all": []}
            continue
        if cur is None:
            continue
        if t.startswith(".Lfunc_end"):
            cur = None
        elif t.endswith(":"):
            blk = []; kern[cur]["blocks"].append(blk)
        elif t and not t.startswith("."):
            blk.append(t); kern[cur]["all"].append(t)
    meta = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+_ZN3srx10k_spectrumILi(\d+)E([fs])E\S*\n.*?\.vgpr_count:\s+(\d+)", text, re.S):
        meta[(int(m.group(2)), m.group(3))] = (int(m.group(4)), int(m.group(1)))
    rows = []
    for (n, t), k in sorted(kern.items()):
        # static counts over the whole kernel: its frame loop is straight-line code (three butterflies per lane and frame at N = 512, two at 64,
        # the twiddle multiplies of the first ones under a lane mask), around it the per-call loads of twiddles, window and row
        ins = k["all"]
        count = lambda *pre: sum(i.startswith(pre) for i in ins)  # noqa: E731
        nb = 3 if n == 512 else 2
        arith = count("v_add_f32", "v_sub_f32", "v_mul_f32", "v_pk_add_f32", "v_pk_mul_f32")
        lds = {}
        for i in ins:
            if i.startswith("ds_"):
                lds[i.split()[0]] = lds.get(i.split()[0], 0) + 1
        rows.append({"kernel": "k_spectrum<%d, %s>" % (n, "float" if t == "f" else "int16_t"), "vgpr_count": meta.get((n, t), (None, None))[0],
                     "lds_bytes": meta.get((n, t), (None, None))[1],
                     "s_barrier": count("s_barrier"),
                     "fused_multiply_adds": sum(bool(re.match(r"v_(pk_)?(fma|fmac|mad|mac)(_mix|_legacy)?_f(16|32|64)", i)) for i in ins),
                     "vector_instructions": count("v_"), "f32_add_sub_mul_instructions": arith, "of_them_packed": count("v_pk_add_f32", "v_pk_mul_f32"),
                     "f32_add_sub_mul_instructions_per_butterfly": round(arith / nb, 1),
                     "lds_instructions": lds,
                     "global_loads": sorted({i.split()[0] for i in ins if i.startswith(("global_load", "s_load", "s_buffer_load"))}),
                     "global_stores": sorted({i.split()[0] for i in ins if i.startswith("global_store")})})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--configs", default="cfg3,cfg2")
    ap.add_argument("--only", default="", help="off: the tap-off rows alone; tap: cfg3 with f32 slots alone (for a kernel trace)")
    ap.add_argument("--isa", action="store_true", help="ISA counts only (no GPU)")
    args = ap.parse_args()
    if args.isa:
        for row in isa_rows():
            print(json.dumps(row), flush=True)
        return
    lib = os.environ.get("SELENITE_RX_LIB", "in-tree")
    for cfg in (["cfg3"] if args.only == "tap" else args.configs.split(",")):
        for q15 in ((False,) if args.only == "tap" else (False, True)):
            med, lo, hi = time_call(cfg, args.iters, q15, None)
            off = med
            print(json.dumps({"config": cfg, "slots": "int16" if q15 else "f32", "tap": "off", "library": lib, "ms_per_call": round(med, 4),
                              "ms_min": round(lo, 4), "ms_max": round(hi, 4), "iters": args.iters}), flush=True)
            if args.only == "off":
                continue
            for tap in TAPS:
                med, lo, hi = time_call(cfg, args.iters, q15, tap)
                rd, wr = tap_bytes(cfg, q15, tap)
                row = {"config": cfg, "slots": "int16" if q15 else "f32", "tap": "N=%d stride=%d" % tap, "ms_per_call": round(med, 4),
                       "ms_min": round(lo, 4), "ms_max": round(hi, 4), "tap_added_ms": round(med - off, 4), "tap_kernel_bytes": rd + wr}
                try:
                    row["d2d_copy_same_bytes_ms"] = round(copy_ms(rd + wr, args.iters), 4)
                except Exception as e:      # (no HIP runtime library where ROCM_PATH says: the yardstick is left out, the row stays)
                    row["d2d_copy_same_bytes_ms"] = None
                    row["d2d_copy_error"] = repr(e)[:80]
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
