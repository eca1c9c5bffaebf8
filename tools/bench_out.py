#!/usr/bin/env python3
"""tools/bench_out.py -- what the audio output stage (selenite_rx_set_out) costs at full size: cfg3 (65 536 channels x 4096 samples, _AUTO)
with the stage off and with L = 4, P = 8 for f32 mono / int16 mono / int16 stereo (and f32 stereo): ms per call (median of --iters launches,
one HIP event between calls, as bench.py takes them), the stage's added ms, for the int16 slots the part of it that is the up-front input
conversion (the int16 call against the f32 call of the same instance shape, stage off and on), the bytes the stage kernel moves, and a
device-to-device copy of the same number of bytes timed in the same process (hipMemcpyAsync of (read + written) / 2 bytes: it reads and writes that many).
--only off: the stage-off rows alone (for an A/B against another build named by SELENITE_RX_LIB); --only stage: the stage-off rows and the f32 mono
stage row alone (a short run for a kernel trace).
--isa: no GPU; compiles csrc/rx_out.hip for gfx950 with the library's flags and reads, per k_out<L, FMT>, the VGPR use, the vector and LDS
instructions of the tap loop per output, whether any fused multiply-add sits in the kernel, and the store widths emitted.
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

FMT = {0: "f32 mono", 1: "f32 stereo", 2: "int16 mono", 3: "int16 stereo"}


def time_call(channels, nsamp, iters, q15, stage, interp=4, plen=8):
    """median ms per call of cfg3 in _AUTO; stage: None or SELENITE_RX_OUT_*"""
    spec = ch.baseline_spec("cfg3", channels, sr.ARITH_AUTO)
    rx = sr.Rx(spec.config())
    if stage is not None:
        rx.set_out(interp, sr.design_interp(interp * plen, interp, 0.4 / interp), stage)
    esz = 2 if q15 else 4
    d_in, d_out = sr.DeviceBuffer(channels * nsamp * 2 * esz), sr.DeviceBuffer(channels * rx.out_values(nsamp) * esz)
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
    vals = rx.out_values(nsamp)
    rx.close()
    d_in.free(); d_out.free()
    return float(np.median(ms)), float(ms.min()), float(ms.max()), vals


def copy_ms(nbytes_read, nbytes_written, iters):
    """a device-to-device copy (hipMemcpyAsync, device to device) that moves the same number of bytes (read + written) as the stage kernel:
    median ms of `iters` copies, one HIP event between copies, in this process"""
    import ctypes as C
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    vp = C.c_void_p
    hip.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    hip.hipEventCreate.argtypes = [C.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    hip.hipEventDestroy.argtypes = [vp]
    n = (nbytes_read + nbytes_written) // 2
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


def isa_rows():
    pkg = os.path.join(ROOT, "selenite-lite_amd")
    flags = subprocess.run(["make", "-s", "-C", pkg, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    flags = [f for f in flags if f != "--offload-compress"] + os.environ.get("BENCH_OUT_EXTRA_FLAGS", "").split()
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "rx_out.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", "-o", asm,
                        os.path.join(pkg, "csrc", "rx_out.hip")], check=True, capture_output=True)
        text = open(asm).read()
    kern, cur, blk = {}, None, None
    for line in text.split("\n"):
        t = line.split(";")[0].strip()
        m = re.match(r"^_ZN3srx5k_outILi(\d+)ELi(\d+)E\S*:$", t)
        if m:
            cur = (int(m.group(1)), int(m.group(2))); blk = []; kern[cur] = {"blocks": [blk], "all": []}
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
    for m in re.finditer(r"\.name:\s+_ZN3srx5k_outILi(\d+)ELi(\d+)E\S*\n(.*?)\.vgpr_count:\s+(\d+)", text, re.S):
        sp = re.search(r"\.sgpr_spill_count:\s+(\d+)", m.group(3))
        meta[(int(m.group(1)), int(m.group(2)))] = (int(m.group(4)), int(sp.group(1)) if sp else 0)
    rows = []
    for (L, fmt), k in sorted(kern.items()):
        K = 16 // {0: 4, 1: 8, 2: 2, 3: 4}[fmt]
        # the tap loop: the basic block with multiplies that branches back to itself
        loops = [b for b in k["blocks"] if any(i.startswith(("v_mul_f32", "v_pk_mul_f32")) for i in b) and any(i.startswith("ds_read") for i in b)
                 and any(i.startswith("s_cbranch") for i in b)]
        body = min(loops, key=len) if loops else []
        vec = [i for i in body if i.startswith(("v_", "ds_", "global_", "buffer_"))]
        stores = {}
        for i in k["all"]:
            if i.startswith("global_store"):
                stores[i.split()[0] + (" nt" if i.rstrip().endswith(" nt") else "")] = stores.get(i.split()[0] + (" nt" if i.rstrip().endswith(" nt") else ""), 0) + 1
        rows.append({"kernel": "k_out<%d, %s>" % (L, FMT[fmt]), "vgpr_count": meta.get((L, fmt), (None, None))[0],
                     "sgpr_spills": meta.get((L, fmt), (None, None))[1],
                     "fused_multiply_adds": sum(bool(re.match(r"v_(pk_)?(fma|fmac|mad|mac)(_mix|_legacy)?_f(16|32|64)", i)) for i in k["all"]),
                     "outputs_per_lane_and_store": K,
                     "tap_loop_vector_instructions_per_tap": len(vec),
                     "tap_loop_lds_reads_per_tap": sum(i.startswith("ds_read") or i.startswith("ds_load") for i in body),
                     "tap_loop_vector_instructions_per_output_and_tap": round(len(vec) / K, 2),
                     "global_stores": stores,
                     "global_loads": sorted({i.split()[0] for i in k["all"] if i.startswith(("global_load", "s_load", "s_buffer_load"))})})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--interp", type=int, default=4)
    ap.add_argument("--phase", type=int, default=8)
    ap.add_argument("--only", default="", help="off: the stage-off rows alone; stage: one f32 mono stage row (for a kernel trace)")
    ap.add_argument("--isa", action="store_true", help="ISA counts only (no GPU)")
    args = ap.parse_args()
    if args.isa:
        for row in isa_rows():
            print(json.dumps(row), flush=True)
        return
    C, N, L, P = args.channels, args.samples, args.interp, args.phase
    lib = os.environ.get("SELENITE_RX_LIB", "in-tree")
    off = {}
    for q15 in (False, True):
        med, lo, hi, _ = time_call(C, N, args.iters, q15, None)
        off[q15] = med
        print(json.dumps({"config": "cfg3", "slots": "int16" if q15 else "f32", "stage": "off", "library": lib, "ms_per_call": round(med, 4),
                          "ms_min": round(lo, 4), "ms_max": round(hi, 4), "iters": args.iters}), flush=True)
    if args.only == "off":
        return
    rows = [(False, sr.OUT_MONO)] if args.only == "stage" else [(False, sr.OUT_MONO), (True, sr.OUT_MONO), (True, sr.OUT_STEREO), (False, sr.OUT_STEREO)]
    f32_added = None
    for q15, frames in rows:
        med, lo, hi, vals = time_call(C, N, args.iters, q15, frames, L, P)
        rd, wr = C * (N // 4) * 4, C * vals * (2 if q15 else 4)       # the stage kernel's bytes: f32 audio in, frames out (state: 4 (P - 1) each way, left out)
        row = {"config": "cfg3", "slots": "int16" if q15 else "f32", "stage": "L=%d P=%d %s" % (L, P, "stereo" if frames else "mono"),
               "ms_per_call": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "stage_added_ms": round(med - off[q15], 4),
               "stage_kernel_bytes": rd + wr, "values_per_channel": vals}
        if not q15 and frames == sr.OUT_MONO:
            f32_added = med - off[False]
        try:
            cp = copy_ms(rd, wr, args.iters)
            row["d2d_copy_same_bytes_ms"] = round(cp, 4)
        except Exception as e:      # (no HIP runtime library where ROCM_PATH says: the yardstick is left out, the row stays)
            row["d2d_copy_same_bytes_ms"] = None
            row["d2d_copy_error"] = repr(e)[:80]
        print(json.dumps(row), flush=True)
    # the up-front conversion of the int16 slots: an int16 call whose chain runs as an f32 call pays k_q15_to_f32 over the input and loses
    # the fused int16 load; measured as (int16 stage-on - int16 stage-off) - (the stage kernel at the same output bytes is not separable here:
    # the kernel trace gives k_q15_to_f32's own time)
    if f32_added is not None:
        print(json.dumps({"note": "int16 rows: stage_added_ms holds the input conversion pass (k_q15_to_f32 in a kernel trace) and the f32 chain kernel in place of the int16 one",
                          "f32_mono_stage_added_ms": round(f32_added, 4)}), flush=True)


if __name__ == "__main__":
    main()
