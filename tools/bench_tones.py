#!/usr/bin/env python3
"""tools/bench_tones.py -- what the tone-detector bank (selenite_rx_set_tones, k_tones<KL>) costs at full size: cfg3 (65 536 channels x 4096
samples, decimated by 4: 268 MB of f32 audio per call) and cfg4 (65 536 x 4096, not decimated: four times the audio), _AUTO, f32 slots:
ms per call (median of --iters launches, one HIP event between calls, as bench.py takes them) with the stage off and with 8, 16, 32 and 64
tones (k_tones<8>, <16>, <32>, <64>; frames of 16 DSP blocks: a call ends one frame), the added ms, and a device-to-device copy
(hipMemcpyAsync, timed in the same process) of the call's audio bytes.  The stage reads those bytes once and writes none of them, the copy
reads and writes them: the copy is an upper bound of the stage's memory floor.  "Added" is more than the stage: with it on the fused kernel
runs with its own AGC off and k_agc_generic reads and writes the audio again (rx_dispatch.hip: run_part).  The input is the synthetic
workload of bench.py; the tones are the first K of the 50 CTCSS frequencies at 12 kHz and 14 more above them.
The kernels' own times are the k_tones / k_agc_generic rows of a kernel trace of the short run:
    rocprofv3 --kernel-trace --stats -- python tools/bench_tones.py --only on --iters 5
--only off: the stage-off rows alone (for an A/B against another build named by SELENITE_RX_LIB); --only on: the stage-on rows alone.
--isa: no GPU; compiles csrc/rx_tones.hip for gfx950 with the library's flags and reads, per k_tones<KL>, VGPRs, SGPRs, LDS and scratch from
the code object's own metadata, counts the vector and LDS instructions of one step of the steady loop and the fused multiply-adds in the
kernel; writes profiles/tones/isa_tones.jsonl.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import selenite_rx as sr  # noqa: E402
from selenite_rx import chain as ch  # noqa: E402

CONFIGS = {"cfg3": ("cfg3", 65536, 4096), "cfg4": ("cfg4", 65536, 4096)}
TONES = (8, 16, 32, 64)
FRAME_BLOCKS = 16


def tone_table(K):
    hz = np.concatenate([sr.ctcss_hz(), 300.0 + 100.0 * np.arange(14)])
    return sr.design_tones(hz[:K] / 12000.0)


def time_call(cfg, iters, K):
    """median ms per call in _AUTO; K: None (off) or the number of tones"""
    name, channels, nsamp = CONFIGS[cfg]
    spec = ch.baseline_spec(name, channels, sr.ARITH_AUTO)
    rx = sr.Rx(spec.config())
    if K is not None:
        rx.set_tones(tone_table(K), frame_blocks=FRAME_BLOCKS, confirm=2, release=2, ratio=0.02, min_power=1e-9)
    d_in, d_out = sr.DeviceBuffer(channels * nsamp * 8), sr.DeviceBuffer(channels * (nsamp // spec.decim) * 4)
    rx.synth_device(d_in.ptr, 0, channels, 0, nsamp, ch.SEED)
    rx.time_process_each(d_in.ptr, d_out.ptr, nsamp, 3, False)
    ms = rx.time_process_each(d_in.ptr, d_out.ptr, nsamp, iters, False)
    rx.sync()
    frames = None
    if K is not None:
        _, power, frames = rx.tones()
        assert np.isfinite(power).all() and frames == (3 + iters) * (nsamp // spec.block) // FRAME_BLOCKS
    rx.close()
    d_in.free(); d_out.free()
    return float(np.median(ms)), float(ms.min()), float(ms.max()), frames


def isa_rows():
    pkg = os.path.join(ROOT, "selenite-lite_amd")
    flags = subprocess.run(["make", "-s", "-C", pkg, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    flags = [f for f in flags if f != "--offload-compress"]
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "rx_tones.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", "-o", asm,
                        os.path.join(pkg, "csrc", "rx_tones.hip")], check=True, capture_output=True)
        text = open(asm).read()

    def label(sym):
        m = re.match(r"^_ZN3srx7k_tonesILi(\d+)EEE", sym)
        return "k_tones<%d>" % int(m.group(1)) if m else None

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
        elif t and (not t.startswith(".") or t.startswith(".LBB")):
            kern[cur].append(t)
    meta = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+(_ZN3srx\S+)\n"
                         r"(?:(?!\.name:).)*?\.private_segment_fixed_size:\s+(\d+)\n(?:(?!\.name:).)*?\.sgpr_count:\s+(\d+)\n"
                         r"(?:(?!\.name:).)*?\.vgpr_count:\s+(\d+)", text, re.S):
        if label(m.group(2)):
            meta[label(m.group(2))] = dict(vgpr_count=int(m.group(5)), sgpr_count=int(m.group(4)), lds_bytes=int(m.group(1)), scratch_bytes=int(m.group(3)))

    def steady_loop(lines):
        """the loop of the unrolled steps: from a label to the branch back to it, the span with the most products c * s1 (one v_mul_f32
        per step; the compiler pairs some of the sums and differences into v_pk_add_f32) and no branch or global access inside"""
        at = {t[:-1]: i for i, t in enumerate(lines) if t.endswith(":")}
        best = None
        for i, t in enumerate(lines):
            m = re.match(r"s_c?branch\S*\s+(\.LBB\S+)", t)
            if m and m.group(1) in at and at[m.group(1)] < i:
                body = [x for x in lines[at[m.group(1)]:i + 1] if not x.endswith(":")]
                if any(x.startswith(("global_", "s_cbranch", "s_branch")) for x in body[:-1]):
                    continue
                muls = sum(x.startswith("v_mul_f32") for x in body)
                if muls and (best is None or muls > sum(x.startswith("v_mul_f32") for x in best)):
                    best = body
        return best

    rows = []
    for k in sorted(kern, key=lambda k: int(re.sub(r"\D", "", k))):
        ins = [t for t in kern[k] if not t.endswith(":")]
        count = lambda *pre: sum(i.startswith(pre) for i in ins)  # noqa: E731
        row = {"kernel": k}
        row.update(meta.get(k, {}))
        loop = steady_loop(kern[k])
        steps = None if loop is None else sum(i.startswith("v_mul_f32") for i in loop)
        row.update({"scratch_instructions": count("scratch_", "buffer_"),
                    "fused_multiply_adds": sum(bool(re.match(r"v_(pk_)?(fma|fmac|mad|mac)(_mix|_legacy)?_f(16|32|64)", i)) for i in ins),
                    "barriers": count("s_barrier"), "vector_instructions": count("v_"), "scalar_instructions": count("s_"), "lds_instructions": count("ds_"),
                    "loop_steps": steps,
                    "step_vector_instructions": None if loop is None else sum(i.startswith("v_") for i in loop) / float(steps),
                    "step_lds_instructions": None if loop is None else sum(i.startswith("ds_") for i in loop) / float(steps),
                    "step_scalar_instructions": None if loop is None else sum(i.startswith("s_") for i in loop) / float(steps),
                    "loop_lds_reads": None if loop is None else sorted({i.split()[0] for i in loop if i.startswith("ds_")}),
                    "global_loads": sorted({i.split()[0] for i in ins if i.startswith("global_load")}),
                    "global_stores": sorted({i.split()[0] for i in ins if i.startswith("global_store")})})
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--configs", default="cfg3,cfg4")
    ap.add_argument("--only", default="", help="off: the stage-off rows alone; on: the stage-on rows alone (for a kernel trace)")
    ap.add_argument("--isa", action="store_true", help="ISA resources only (no GPU); also written to profiles/tones/isa_tones.jsonl")
    args = ap.parse_args()
    if args.isa:
        out = os.path.join(ROOT, "profiles", "tones", "isa_tones.jsonl")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            for row in isa_rows():
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
        return
    from bench_meter import copy_ms
    lib = os.environ.get("SELENITE_RX_LIB", "in-tree")
    for cfg in args.configs.split(","):
        name, channels, nsamp = CONFIGS[cfg]
        audio_bytes = channels * (nsamp // ch.baseline_spec(name, 1).decim) * 4      # the un-scaled f32 audio of a call: what k_tones reads
        off = None
        if args.only != "on":
            off, lo, hi, _ = time_call(cfg, args.iters, None)
            print(json.dumps({"config": cfg, "tones": "off", "library": lib, "ms_per_call": round(off, 4), "ms_min": round(lo, 4),
                              "ms_max": round(hi, 4), "iters": args.iters}), flush=True)
        if args.only == "off":
            continue
        try:
            cp, err = copy_ms(audio_bytes, args.iters), None
        except Exception as e:      # (no HIP runtime library where ROCM_PATH says: the yardstick is left out, the rows stay)
            cp, err = None, repr(e)[:80]
        for K in TONES:
            med, lo, hi, frames = time_call(cfg, args.iters, K)
            row = {"config": cfg, "tones": "n_tones=%d" % K, "ms_per_call": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                   "audio_bytes": audio_bytes, "frames": frames, "recurrence_steps": channels * K * (audio_bytes // 4 // channels)}
            if cp is not None:
                row["d2d_copy_audio_bytes_ms"] = round(cp, 4)
            if off is not None:
                row["added_ms"] = round(med - off, 4)
                row["call_over_off"] = round(med / off, 3)
            if err:
                row["d2d_copy_error"] = err
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
