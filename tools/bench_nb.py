#!/usr/bin/env python3
"""tools/bench_nb.py -- what the impulse noise blanker (selenite_rx_set_nb) costs at full size: cfg3 (65 536 channels x 4096 samples, _AUTO), f32
and int16 slots, with the stage off and with F = 32, 64 and 128 (guard 2, max_hits 8, threshold 8, alpha 0.125, clamp 2): ms per call (median of
--iters launches, one HIP event between calls, as bench.py takes them), the stage's added ms, and a device-to-device copy of the call's input
bytes timed in the same process (hipMemcpyAsync: the stage reads and writes the input once, so that copy is its floor).  The stage kernel's
own time is the k_nb row of a kernel trace of the short run:
    rocprofv3 --kernel-trace --stats -- python tools/bench_nb.py --only nb --iters 5
--only off: the stage-off rows alone (for an A/B against another build named by SELENITE_RX_LIB); --only nb: the F = 64 rows alone.
--isa: no GPU; compiles csrc/rx_nb.hip for gfx950 with the library's flags and reads, per k_nb<F, TIn>, the VGPR use, the LDS image, and
whether any fused multiply-add or division sits in the kernel.
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
FRAMES = (32, 64, 128)


def time_call(cfg, iters, q15, frame):
    """median ms per call in _AUTO; frame: None (stage off) or F"""
    name, channels, nsamp = CONFIGS[cfg]
    spec = ch.baseline_spec(name, channels, sr.ARITH_AUTO)
    rx = sr.Rx(spec.config())
    if frame is not None:
        rx.set_nb(frame)
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
    counts = None
    if frame is not None:
        st = rx.nb_state()
        counts = (int(st["blanked"].sum()), int(st["bursts"].sum()))
    rx.close()
    d_in.free(); d_out.free()
    return float(np.median(ms)), float(ms.min()), float(ms.max()), counts


def copy_ms(nbytes, iters):
    """a device-to-device copy (hipMemcpyAsync) of `nbytes` (read once, written once): median ms of `iters` copies, one HIP event between
    copies, in this process"""
    import ctypes as C
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    vp = C.c_void_p
    hip.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    hip.hipEventCreate.argtypes = [C.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    hip.hipEventDestroy.argtypes = [vp]
    a, b = sr.DeviceBuffer(nbytes), sr.DeviceBuffer(nbytes)
    ev = [vp() for _ in range(iters + 1)]
    for e in ev:
        if hip.hipEventCreate(C.byref(e)):
            raise RuntimeError("hipEventCreate")
    d2d = 3                                                  # hipMemcpyDeviceToDevice
    for _ in range(3):
        hip.hipMemcpyAsync(b.ptr, a.ptr, nbytes, d2d, None)
    hip.hipEventRecord(ev[0], None)
    for i in range(iters):
        if hip.hipMemcpyAsync(b.ptr, a.ptr, nbytes, d2d, None):
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


def isa_rows():
    pkg = os.path.join(ROOT, "selenite-lite_amd")
    flags = subprocess.run(["make", "-s", "-C", pkg, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    flags = [f for f in flags if f != "--offload-compress"] + os.environ.get("BENCH_NB_EXTRA_FLAGS", "").split()
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "rx_nb.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", "-o", asm,
                        os.path.join(pkg, "csrc", "rx_nb.hip")], check=True, capture_output=True)
        text = open(asm).read()
    kern, cur = {}, None
    for line in text.split("\n"):
        t = line.split(";")[0].strip()
        m = re.match(r"^_ZN3srx4k_nbILi(\d+)E([fs])E\S*:$", t)
        if m:
            cur = (int(m.group(1)), m.group(2)); kern[cur] = []
            continue
        if cur is None:
            continue
        if t.startswith(".Lfunc_end"):
            cur = None
        elif t and not t.startswith(".") and not t.endswith(":"):
            kern[cur].append(t)
    meta = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+_ZN3srx4k_nbILi(\d+)E([fs])E\S*\n.*?\.vgpr_count:\s+(\d+)", text, re.S):
        meta[(int(m.group(2)), m.group(3))] = (int(m.group(4)), int(m.group(1)))
    rows = []
    for (n, t), ins in sorted(kern.items()):
        count = lambda *pre: sum(i.startswith(pre) for i in ins)  # noqa: E731
        rows.append({"kernel": "k_nb<%d, %s>" % (n, "float" if t == "f" else "int16_t"), "vgpr_count": meta.get((n, t), (None, None))[0],
                     "lds_bytes": meta.get((n, t), (None, None))[1],
                     "fused_multiply_adds": sum(bool(re.match(r"v_(pk_)?(fma|fmac|mad|mac)(_mix|_legacy)?_f(16|32|64)", i)) for i in ins),
                     "divisions": count("v_rcp", "v_div"),
                     "vector_instructions": count("v_"), "scalar_instructions": count("s_"), "lds_instructions": count("ds_"),
                     "global_loads": sorted({i.split()[0] for i in ins if i.startswith("global_load")}),
                     "global_stores": sorted({i.split()[0] for i in ins if i.startswith("global_store")})})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--configs", default="cfg3")
    ap.add_argument("--only", default="", help="off: the stage-off rows alone; nb: F = 64 alone (for a kernel trace)")
    ap.add_argument("--isa", action="store_true", help="ISA counts only (no GPU)")
    args = ap.parse_args()
    if args.isa:
        for row in isa_rows():
            print(json.dumps(row), flush=True)
        return
    lib = os.environ.get("SELENITE_RX_LIB", "in-tree")
    for cfg in args.configs.split(","):
        _, channels, nsamp = CONFIGS[cfg]
        for q15 in (False, True):
            nbytes = channels * nsamp * (4 if q15 else 8)
            off = None
            if args.only != "nb":
                off, lo, hi, _ = time_call(cfg, args.iters, q15, None)
                print(json.dumps({"config": cfg, "slots": "int16" if q15 else "f32", "nb": "off", "library": lib, "ms_per_call": round(off, 4),
                                  "ms_min": round(lo, 4), "ms_max": round(hi, 4), "iters": args.iters}), flush=True)
            if args.only == "off":
                continue
            try:
                cp, err = copy_ms(nbytes, args.iters), None
            except Exception as e:      # (no HIP runtime library where ROCM_PATH says: the yardstick is left out, the rows stay)
                cp, err = None, repr(e)[:80]
            for frame in ((64,) if args.only == "nb" else FRAMES):
                med, lo, hi, counts = time_call(cfg, args.iters, q15, frame)
                row = {"config": cfg, "slots": "int16" if q15 else "f32", "nb": "F=%d" % frame, "ms_per_call": round(med, 4), "ms_min": round(lo, 4),
                       "ms_max": round(hi, 4), "input_bytes": nbytes, "d2d_copy_input_bytes_ms": round(cp, 4) if cp is not None else None,
                       "blanked": counts[0], "bursts": counts[1]}
                if off is not None:
                    row["nb_added_ms"] = round(med - off, 4)
                    if cp:
                        row["added_over_copy"] = round((med - off) / cp, 3)
                if err:
                    row["d2d_copy_error"] = err
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
