#!/usr/bin/env python3
"""tools/bench_iqc.py -- what the I/Q correction stage (selenite_rx_set_iqc) costs at full size: cfg3 (65 536 channels x 4096 samples, _AUTO), f32
and int16 slots, with the stage off and with F = 32, 64 and 128 (alpha 1/64, dc_alpha 1/16, p_max 0.25, g_max 1.5, min_power 1e-12): ms per
call (median of --iters launches, one HIP event between calls, as bench.py takes them), the stage's added ms, and device-to-device copies
timed in the same process (hipMemcpyAsync) of the bytes the stage moves: with f32 slots it reads the input bytes and writes as many, so a
copy of the input bytes is its floor; with int16 slots it reads 1.07 GB and writes 2.15 GB, which a copy of 1.07 GB and one of 2.15 GB
bracket.  With int16 slots "added" also holds the f32-in / int16-out route of the chain behind the stage (the fused kernel with its AGC
off, then k_agc_generic).  The stage kernel's own time is the k_iqc row of a kernel trace of the short run:
    rocprofv3 --kernel-trace --stats -- python tools/bench_iqc.py --only iqc --iters 5
--only off: the stage-off rows alone (for an A/B against another build named by SELENITE_RX_LIB); --only iqc: the F = 64 rows alone.
--isa: no GPU; compiles csrc/rx_iqc.hip for gfx950 with the library's flags and reads, per k_iqc<F, TIn>, the VGPR use, the LDS image,
scratch, and whether any fused multiply-add sits in the kernel; writes profiles/iqc/isa_iqc.jsonl.
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
        rx.set_iqc(frame)
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
        counts = int(rx.iqc_state()["held"].sum())
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
    flags = [f for f in flags if f != "--offload-compress"] + os.environ.get("BENCH_IQC_EXTRA_FLAGS", "").split()
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "rx_iqc.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", "-o", asm,
                        os.path.join(pkg, "csrc", "rx_iqc.hip")], check=True, capture_output=True)
        text = open(asm).read()
    kern, cur = {}, None
    for line in text.split("\n"):
        t = line.split(";")[0].strip()
        m = re.match(r"^_ZN3srx5k_iqcILi(\d+)E([fs])E\S*:$", t)
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
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+_ZN3srx5k_iqcILi(\d+)E([fs])E\S*\n"
                         r"(?:(?!\.name:).)*?\.private_segment_fixed_size:\s+(\d+)\n(?:(?!\.name:).)*?\.vgpr_count:\s+(\d+)", text, re.S):
        meta[(int(m.group(2)), m.group(3))] = (int(m.group(5)), int(m.group(1)), int(m.group(4)))
    rows = []
    for (n, t), ins in sorted(kern.items()):
        count = lambda *pre: sum(i.startswith(pre) for i in ins)  # noqa: E731
        vgpr, lds, scratch = meta.get((n, t), (None, None, None))
        # a correctly rounded division is v_div_scale .. v_div_fixup with five fused multiply-adds inside, a correctly rounded square root
        # v_sqrt_f32 and two behind it within a dozen instructions: those belong to the operation; any other one would be a contraction
        fma_all, fma_op, in_div, sqrt_left = 0, 0, False, 0
        for i in ins:
            if i.startswith("v_div_scale_f32"):
                in_div = True
            elif i.startswith("v_div_fixup_f32"):
                in_div = False
            elif i.startswith("v_sqrt_f32"):
                sqrt_left = 12
            elif re.match(r"v_(pk_)?(fma|fmac|mad|mac)(_mix|_legacy)?_f(16|32|64)", i):
                fma_all += 1
                fma_op += 1 if in_div or sqrt_left > 0 else 0
            sqrt_left -= 1
        rows.append({"kernel": "k_iqc<%d, %s>" % (n, "float" if t == "f" else "int16_t"), "vgpr_count": vgpr, "lds_bytes": lds,
                     "scratch_bytes": scratch, "scratch_instructions": count("scratch_", "buffer_"),
                     "fused_multiply_adds": fma_all - fma_op, "fma_inside_division_and_sqrt": fma_op,
                     "divisions": count("v_div_fixup"), "square_roots": count("v_sqrt"), "approximate_rcp_rsq_alone": count("v_rsq") + count("v_rcp") - count("v_div_fixup"),
                     "vector_instructions": count("v_"), "scalar_instructions": count("s_"), "lds_instructions": count("ds_"),
                     "global_loads": sorted({i.split()[0] for i in ins if i.startswith("global_load")}),
                     "global_stores": sorted({i.split()[0] for i in ins if i.startswith("global_store")})})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--configs", default="cfg3")
    ap.add_argument("--only", default="", help="off: the stage-off rows alone; iqc: F = 64 alone (for a kernel trace)")
    ap.add_argument("--isa", action="store_true", help="ISA counts only (no GPU); also written to profiles/iqc/isa_iqc.jsonl")
    args = ap.parse_args()
    if args.isa:
        out = os.path.join(ROOT, "profiles", "iqc", "isa_iqc.jsonl")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            for row in isa_rows():
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
        return
    lib = os.environ.get("SELENITE_RX_LIB", "in-tree")
    for cfg in args.configs.split(","):
        _, channels, nsamp = CONFIGS[cfg]
        for q15 in (False, True):
            nin, nout = channels * nsamp * (4 if q15 else 8), channels * nsamp * 8      # the stage reads nin bytes and writes nout
            off = None
            if args.only != "iqc":
                off, lo, hi, _ = time_call(cfg, args.iters, q15, None)
                print(json.dumps({"config": cfg, "slots": "int16" if q15 else "f32", "iqc": "off", "library": lib, "ms_per_call": round(off, 4),
                                  "ms_min": round(lo, 4), "ms_max": round(hi, 4), "iters": args.iters}), flush=True)
            if args.only == "off":
                continue
            try:
                cp, err = {n: copy_ms(n, args.iters) for n in sorted({nin, nout})}, None
            except Exception as e:      # (no HIP runtime library where ROCM_PATH says: the yardstick is left out, the rows stay)
                cp, err = {}, repr(e)[:80]
            for frame in ((64,) if args.only == "iqc" else FRAMES):
                med, lo, hi, held = time_call(cfg, args.iters, q15, frame)
                row = {"config": cfg, "slots": "int16" if q15 else "f32", "iqc": "F=%d" % frame, "ms_per_call": round(med, 4), "ms_min": round(lo, 4),
                       "ms_max": round(hi, 4), "bytes_read": nin, "bytes_written": nout, "held": held}
                for n, ms in cp.items():
                    row["d2d_copy_%d_bytes_ms" % n] = round(ms, 4)
                if off is not None:
                    row["iqc_added_ms"] = round(med - off, 4)
                    for n, ms in cp.items():
                        row["added_over_copy_%d" % n] = round((med - off) / ms, 3)
                if err:
                    row["d2d_copy_error"] = err
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
