#!/usr/bin/env python3
"""tools/bench_meter.py -- what the signal-level meter and squelch (selenite_rx_set_meter) costs at full size: cfg3 (65 536 channels x 4096
samples, 16 DSP blocks of 64 audio samples per channel and call) and cfg2 (4096 channels x 48 000 samples, 375 blocks of 128), _AUTO, f32 and
int16 slots: ms per call (median of --iters launches, one HIP event between calls, as bench.py takes them) with the stage off, as a meter
(gate = 0) and as a squelch (gate = 1), the stage's added ms, and a device-to-device copy (hipMemcpyAsync, timed in the same process) of the
call's audio bytes, 4 bytes per audio sample: the stage itself reads those once.  "Added" is more than the stage: with it on the fused kernel
runs with its own AGC off and k_agc_generic reads and writes the audio again (rx_dispatch.hip: run_part).  The input is the synthetic
workload of bench.py; the thresholds sit below most of its block powers (the row says how many blocks were open).
The kernels' own times are the k_meter / k_gate / k_agc_generic rows of a kernel trace of the short run:
    rocprofv3 --kernel-trace --stats -- python tools/bench_meter.py --only meter --iters 5
--only off: the stage-off rows alone (for an A/B against another build named by SELENITE_RX_LIB); --only meter: the gate = 1 rows alone.
--isa: no GPU; compiles csrc/rx_meter.hip for gfx950 with the library's flags and reads, per k_meter<B> and k_gate<TOut>, VGPRs, SGPRs, LDS
and scratch from the code object's own metadata, and counts fused multiply-adds outside the correctly rounded division (and outside the compiler's u32 division); writes profiles/meter/isa_meter.jsonl.
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
# the level of the synthetic workload's un-scaled audio (three tones and noise) has its median over the channels at 0.31 (cfg3) and 0.34 (cfg2);
# with these thresholds nearly every block is open (the rows say how many), so k_gate reads its bytes and writes next to nothing
PAR = dict(sense=sr.SQ_ABOVE, hang=2, attack=0.5, decay=0.5, open_level=0.12, close_level=0.08, level_init=0.0)


def time_call(cfg, iters, q15, gate):
    """median ms per call in _AUTO; gate: None (stage off), 0 (meter only) or 1"""
    name, channels, nsamp = CONFIGS[cfg]
    spec = ch.baseline_spec(name, channels, sr.ARITH_AUTO)
    rx = sr.Rx(spec.config())
    if gate is not None:
        rx.set_meter(gate=gate, **PAR)
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
    if gate is not None:
        st = rx.meter_state()
        blocks = (iters + 3) * channels * (nsamp // spec.block)
        counts = dict(open_share=round(float(st["open_blocks"].sum()) / blocks, 4), opens=int(st["opens"].sum()),
                      level_median=float(np.median(st["level"])))
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
    flags = [f for f in flags if f != "--offload-compress"]
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "rx_meter.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", "-o", asm,
                        os.path.join(pkg, "csrc", "rx_meter.hip")], check=True, capture_output=True)
        text = open(asm).read()

    def label(sym):
        m = re.match(r"^_ZN3srx7k_meterILi(\d+)EEE", sym)
        if m:
            return "k_meter<%d>" % int(m.group(1))
        m = re.match(r"^_ZN3srx6k_gateI([fs])EE", sym)
        return "k_gate<%s>" % ("float" if m.group(1) == "f" else "int16_t") if m else None

    kern, cur = {}, None
    for line in text.split("\n"):
        t = line.split(";")[0].strip()
        m = re.match(r"^(_ZN3srx\S+):$", t)
        if m and label(m.group(1)):
            cur = label(m.group(1)); kern[cur] = []
            continue
        if cur is None:
            continue
        if t.startswith(".Lfunc_end"):
            cur = None
        elif t and not t.startswith(".") and not t.endswith(":"):
            kern[cur].append(t)
    meta = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+(_ZN3srx\S+)\n"
                         r"(?:(?!\.name:).)*?\.private_segment_fixed_size:\s+(\d+)\n(?:(?!\.name:).)*?\.sgpr_count:\s+(\d+)\n"
                         r"(?:(?!\.name:).)*?\.vgpr_count:\s+(\d+)", text, re.S):
        if label(m.group(2)):
            meta[label(m.group(2))] = dict(vgpr_count=int(m.group(5)), sgpr_count=int(m.group(4)), lds_bytes=int(m.group(1)), scratch_bytes=int(m.group(3)))
    rows = []
    order = lambda k: (k.startswith("k_gate"), int(re.sub(r"\D", "", k) or 0), k)  # noqa: E731
    for k in sorted(kern, key=order):
        ins = kern[k]
        count = lambda *pre: sum(i.startswith(pre) for i in ins)  # noqa: E731
        # the correctly rounded division is v_div_scale .. v_div_fixup with fused multiply-adds inside: those belong to the operation
        # (and the compiler's u32 division of the magic constant goes through v_rcp_iflag_f32 and one v_fma_f32 behind it: integer arithmetic)
        fma_all, fma_div, fma_int, in_div, int_left = 0, 0, 0, False, 0
        for i in ins:
            if i.startswith("v_div_scale_f32"):
                in_div = True
            elif i.startswith("v_div_fixup_f32"):
                in_div = False
            elif i.startswith("v_rcp_iflag_f32"):
                int_left = 8
            elif re.match(r"v_(pk_)?(fma|fmac|mad|mac)(_mix|_legacy)?_f(16|32|64)", i):
                fma_all += 1
                fma_div += 1 if in_div else 0
                fma_int += 1 if int_left > 0 and not in_div else 0
            int_left -= 1
        row = {"kernel": k}
        row.update(meta.get(k, {}))
        row.update({"scratch_instructions": count("scratch_", "buffer_"), "fused_multiply_adds": fma_all - fma_div - fma_int, "fma_inside_division": fma_div, "fma_inside_integer_division": fma_int,
                    "divisions": count("v_div_fixup"), "barriers": count("s_barrier"), "vector_instructions": count("v_"),
                    "scalar_instructions": count("s_"), "lds_instructions": count("ds_"),
                    "global_loads": sorted({i.split()[0] for i in ins if i.startswith("global_load")}),
                    "global_stores": sorted({i.split()[0] for i in ins if i.startswith("global_store")})})
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--configs", default="cfg3,cfg2")
    ap.add_argument("--only", default="", help="off: the stage-off rows alone; meter: gate = 1 alone (for a kernel trace)")
    ap.add_argument("--isa", action="store_true", help="ISA resources only (no GPU); also written to profiles/meter/isa_meter.jsonl")
    args = ap.parse_args()
    if args.isa:
        out = os.path.join(ROOT, "profiles", "meter", "isa_meter.jsonl")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            for row in isa_rows():
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
        return
    lib = os.environ.get("SELENITE_RX_LIB", "in-tree")
    for cfg in args.configs.split(","):
        name, channels, nsamp = CONFIGS[cfg]
        audio_bytes = channels * (nsamp // ch.baseline_spec(name, 1).decim) * 4      # the un-scaled f32 audio of a call: what k_meter reads
        for q15 in (False, True):
            off = None
            if args.only != "meter":
                off, lo, hi, _ = time_call(cfg, args.iters, q15, None)
                print(json.dumps({"config": cfg, "slots": "int16" if q15 else "f32", "meter": "off", "library": lib, "ms_per_call": round(off, 4),
                                  "ms_min": round(lo, 4), "ms_max": round(hi, 4), "iters": args.iters}), flush=True)
            if args.only == "off":
                continue
            try:
                cp, err = copy_ms(audio_bytes, args.iters), None
            except Exception as e:      # (no HIP runtime library where ROCM_PATH says: the yardstick is left out, the rows stay)
                cp, err = None, repr(e)[:80]
            for gate in ((1,) if args.only == "meter" else (0, 1)):
                med, lo, hi, counts = time_call(cfg, args.iters, q15, gate)
                row = {"config": cfg, "slots": "int16" if q15 else "f32", "meter": "gate=%d" % gate, "ms_per_call": round(med, 4),
                       "ms_min": round(lo, 4), "ms_max": round(hi, 4), "audio_bytes": audio_bytes}
                row.update(counts)
                if cp is not None:
                    row["d2d_copy_audio_bytes_ms"] = round(cp, 4)
                if off is not None:
                    row["added_ms"] = round(med - off, 4)
                    row["call_over_off"] = round(med / off, 3)
                    if cp is not None:
                        row["added_over_copy"] = round((med - off) / cp, 2)
                if err:
                    row["d2d_copy_error"] = err
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
