#!/usr/bin/env python3
"""tools/bench_fskdec.py -- what the FSK teleprinter decoder (selenite_rx_set_fskdec) costs at the cfg3- and cfg4-size calls (65 536 channels
x 4096 samples: 1024 / 4096 audio samples per channel and call), _AUTO, f32 slots: ms per call (median of --iters launches, one HIP event
between calls, as bench.py takes them) with the stage off and on, the added ms, and a device-to-device copy (hipMemcpyAsync, timed in the
same process) of the call's audio bytes.  The stage reads those bytes once and writes none of them, the copy reads and writes them: the copy
is an upper bound of the stage's memory floor.  "Added" is more than the stage: with it on the fused kernel runs with its own AGC off and
k_agc_generic reads and writes the audio again (rx_dispatch.hip: run_part).  The input is the synthetic workload of bench.py; with frac and
min_power at 0 any audio moves the level, so the bit clocks run and characters are emitted; the row says how many.
The kernels' own times are the k_fskdec / k_cwdec / k_tones<8> rows of a kernel trace of a short run with the Morse decoder and an 8-tone bank
on beside the stage, all three over the same audio:
    rocprofv3 --kernel-trace --stats -- python tools/bench_fskdec.py --only on --with-neighbours --configs cfg4 --iters 5
--only off: the stage-off rows alone (for an A/B against another build named by SELENITE_RX_LIB); --only on: the stage-on rows alone.
--isa: no GPU; compiles csrc/rx_fskdec.hip for gfx950 with the library's flags and reads k_fskdec's VGPRs, SGPRs, LDS and scratch from the code
object's own metadata, finds the loop of the unrolled steps and counts its instructions per step, and counts fused multiply-adds; writes
profiles/fskdec/isa_fskdec.jsonl.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import selenite_rx as sr  # noqa: E402
from selenite_rx import chain as ch  # noqa: E402

CONFIGS = {"cfg3": ("cfg3", 65536, 4096), "cfg4": ("cfg4", 65536, 4096)}
FS = 12000.0
# mark, space and bandwidth in cycles per audio sample: the RTTY pair at cfg3's 12 kHz of audio; a 170 Hz pair around the pitch of cfg4's CW
# filter (500 Hz at 48 kHz), where that chain's audio is
TONES = {"cfg3": (2125.0 / FS, 2295.0 / FS, 140.0 / FS), "cfg4": (415.0 / 48000.0, 585.0 / 48000.0, 140.0 / 48000.0)}
PAR = dict(tick=16, bit_q8=8 * 256, frac=0.0, min_power=0.0)
PRODUCTS_PER_STEP = 6                            # five coefficient products and the square of the outputs: v_pk_mul_f32 each


def time_call(cfg, iters, on, neighbours):
    """median ms per call in _AUTO"""
    name, channels, nsamp = CONFIGS[cfg]
    spec = ch.baseline_spec(name, channels, sr.ARITH_AUTO)
    rx = sr.Rx(spec.config())
    if on:
        mark, space = sr.fsk_bandpass(*TONES[cfg])
        rx.set_fskdec(mark, space, **PAR)
    if neighbours:
        rx.set_cwdec(debounce=1, unit_min=256, unit_init=256, unit_max=16 * 256)
        rx.set_tones(sr.design_tones(sr.ctcss_hz()[:8] / FS), frame_blocks=16, confirm=2, release=2, ratio=0.02, min_power=1e-9)
    d_in, d_out = sr.DeviceBuffer(channels * nsamp * 8), sr.DeviceBuffer(channels * (nsamp // spec.decim) * 4)
    rx.synth_device(d_in.ptr, 0, channels, 0, nsamp, ch.SEED)
    rx.time_process_each(d_in.ptr, d_out.ptr, nsamp, 3, False)
    ms = rx.time_process_each(d_in.ptr, d_out.ptr, nsamp, iters, False)
    rx.sync()
    counts = None
    if on:
        _, count, ferr, lvl = rx.fskdec()
        counts = dict(characters=int(count.sum()), channels_with_text=int((count > 0).sum()), framing_errors=int(ferr.sum()))
    rx.close()
    d_in.free(); d_out.free()
    return float(np.median(ms)), float(ms.min()), float(ms.max()), counts


def isa_rows():
    pkg = os.path.join(ROOT, "selenite-lite_amd")
    flags = subprocess.run(["make", "-s", "-C", pkg, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    flags = [f for f in flags if f != "--offload-compress"]
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "rx_fskdec.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", "-o", asm,
                        os.path.join(pkg, "csrc", "rx_fskdec.hip")], check=True, capture_output=True)
        text = open(asm).read()
    lines, cur = [], False
    for line in text.split("\n"):
        t = line.split(";")[0].strip()
        if re.match(r"^_ZN3srx8k_fskdecE\S+:$", t):
            cur = True
            continue
        if not cur:
            continue
        if t.startswith(".Lfunc_end"):
            break
        if t and (not t.startswith(".") or t.startswith(".LBB")):
            lines.append(t)
    m = re.search(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+_ZN3srx8k_fskdecE\S+\n"
                  r"(?:(?!\.name:).)*?\.private_segment_fixed_size:\s+(\d+)\n(?:(?!\.name:).)*?\.sgpr_count:\s+(\d+)\n"
                  r"(?:(?!\.name:).)*?\.vgpr_count:\s+(\d+)", text, re.S)
    row = {"kernel": "k_fskdec"}
    if m:
        row.update(vgpr_count=int(m.group(4)), sgpr_count=int(m.group(3)), lds_bytes=int(m.group(1)), scratch_bytes=int(m.group(2)))
    # the loop of the unrolled steps: from a label to the branch back to it, the span with the most packed products and no global access
    at = {t[:-1]: i for i, t in enumerate(lines) if t.endswith(":")}
    loop = None
    for i, t in enumerate(lines):
        b = re.match(r"s_c?branch\S*\s+(\.LBB\S+)", t)
        if b and b.group(1) in at and at[b.group(1)] < i:
            body = [x for x in lines[at[b.group(1)]:i + 1] if not x.endswith(":")]
            if any(x.startswith(("global_", "s_cbranch", "s_branch")) for x in body[:-1]):
                continue
            muls = sum(x.startswith("v_pk_mul_f32") for x in body)
            if muls and (loop is None or muls > sum(x.startswith("v_pk_mul_f32") for x in loop)):
                loop = body
    ins = [t for t in lines if not t.endswith(":")]
    count = lambda *pre: sum(i.startswith(pre) for i in ins)  # noqa: E731
    fma = r"v_(pk_)?(fma|fmac|mad|mac)(_mix|_legacy)?_f(16|32|64)"
    steps = None if loop is None else sum(i.startswith("v_pk_mul_f32") for i in loop) / float(PRODUCTS_PER_STEP)
    row.update({"scratch_instructions": count("scratch_", "buffer_"), "fused_multiply_adds": sum(bool(re.match(fma, i)) for i in ins),
                "barriers": count("s_barrier"), "vector_instructions": count("v_"), "scalar_instructions": count("s_"), "lds_instructions": count("ds_"),
                "packed_multiplies": count("v_pk_mul_f32"), "packed_adds": count("v_pk_add_f32"),
                "loop_steps": steps,
                "loop_fused_multiply_adds": None if loop is None else sum(bool(re.match(fma, i)) for i in loop),
                "step_vector_instructions": None if loop is None else sum(i.startswith("v_") for i in loop) / steps,
                "step_packed_instructions": None if loop is None else sum(i.startswith("v_pk_") for i in loop) / steps,
                "step_lds_instructions": None if loop is None else sum(i.startswith("ds_") for i in loop) / steps,
                "step_scalar_instructions": None if loop is None else sum(i.startswith("s_") for i in loop) / steps,
                "loop_lds_reads": None if loop is None else sorted({i.split()[0] for i in loop if i.startswith("ds_")}),
                "global_loads": sorted({i.split()[0] for i in ins if i.startswith("global_load")}),
                "global_stores": sorted({i.split()[0] for i in ins if i.startswith("global_store")})})
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--configs", default="cfg3,cfg4")
    ap.add_argument("--only", default="", help="off: the stage-off rows alone; on: the stage-on rows alone (for a kernel trace)")
    ap.add_argument("--with-neighbours", action="store_true", help="the Morse decoder and an 8-tone bank on in every row: k_cwdec and k_tones<8> next to k_fskdec in a trace")
    ap.add_argument("--isa", action="store_true", help="ISA resources only (no GPU); also written to profiles/fskdec/isa_fskdec.jsonl")
    args = ap.parse_args()
    if args.isa:
        out = os.path.join(ROOT, "profiles", "fskdec", "isa_fskdec.jsonl")
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
        spec = ch.baseline_spec(name, 1)
        audio_bytes = channels * (nsamp // spec.decim) * 4              # the un-scaled f32 audio of a call: what k_fskdec reads
        base = {"config": cfg, "channels": channels, "samples": nsamp, "audio_samples": nsamp // spec.decim, "tick": PAR["tick"],
                "neighbours": bool(args.with_neighbours), "library": lib, "iters": args.iters}
        off = None
        if args.only != "on":
            off, lo, hi, _ = time_call(cfg, args.iters, False, args.with_neighbours)
            print(json.dumps(dict(base, fskdec="off", ms_per_call=round(off, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))), flush=True)
        if args.only == "off":
            continue
        med, lo, hi, counts = time_call(cfg, args.iters, True, args.with_neighbours)
        row = dict(base, fskdec="on", ms_per_call=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), audio_bytes=audio_bytes,
                   steps_per_wave=nsamp // spec.decim)
        row.update(counts)
        try:
            row["d2d_copy_audio_bytes_ms"] = round(copy_ms(audio_bytes, args.iters), 4)
        except Exception as e:      # (no HIP runtime library where ROCM_PATH says: the yardstick is left out, the rows stay)
            row["d2d_copy_error"] = repr(e)[:80]
        if off is not None:
            row["added_ms"] = round(med - off, 4)
            row["call_over_off"] = round(med / off, 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
