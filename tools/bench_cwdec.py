#!/usr/bin/env python3
"""tools/bench_cwdec.py -- what the Morse decoder (selenite_rx_set_cwdec) costs at a given shape, by default the cfg4-size call (65 536
channels x 4096 samples: 16 DSP blocks of 256 audio samples per channel and call), _AUTO, f32 and int16 slots: ms per call (median of
--iters launches, one HIP event between calls, as bench.py takes them) with the stage off and on, and the added ms.  "Added" is more than
the stage: with it on the fused kernel runs with its own AGC off and k_agc_generic reads and writes the audio again (rx_dispatch.hip:
run_part).  The input is the synthetic workload of bench.py under a per-channel on / off pattern of whole DSP blocks (marks of 1 - 3 blocks,
the same 16 blocks in every call), so the decoder keys, times elements and emits characters; the row says how many.
The kernels' own times are the k_cwdec / k_meter / k_agc_generic rows of a kernel trace of a short run with the meter on beside the decoder,
both over the same audio:
    rocprofv3 --kernel-trace --stats -- python tools/bench_cwdec.py --only on --with-meter --slots f32 --iters 5
--only off: the stage-off rows alone (for an A/B against another build named by SELENITE_RX_LIB); --only on: the stage-on rows alone.
--isa: no GPU; compiles csrc/rx_cwdec.hip for gfx950 with the library's flags and reads, per k_cwdec<B>, VGPRs, SGPRs, LDS and scratch from
the code object's own metadata, and counts fused multiply-adds outside the correctly rounded division (and outside the compiler's u32
divisions); writes profiles/cwdec/isa_cwdec.jsonl.
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

# DSP blocks of 256 samples at 12 kHz are 21 ms: a unit of one to three blocks
PAR = dict(debounce=1, unit_min=256, unit_init=256, unit_max=16 * 256, track=2, ring=256)
METER = dict(sense=sr.SQ_ABOVE, gate=0, hang=2, attack=0.5, decay=0.5, open_level=0.12, close_level=0.08, level_init=0.0)


def keyed_input(rx, spec, channels, nsamp, q15):
    """the synthetic workload under a per-channel pattern of whole DSP blocks: 1 down, 0.03 up"""
    blocks = nsamp // spec.block
    rng = np.random.default_rng(7)
    pat = np.zeros((channels, blocks), np.float32)
    for c0 in range(0, channels, 4096):
        p = rng.integers(0, 2, (min(4096, channels - c0), (blocks + 1) // 2))
        pat[c0:c0 + p.shape[0]] = np.repeat(p, 2, axis=1)[:, :blocks]              # marks and spaces of two blocks and more
    env = np.where(pat > 0, np.float32(1.0), np.float32(0.03))
    f = sr.DeviceBuffer(channels * nsamp * 8)
    rx.synth_device(f.ptr, 0, channels, 0, nsamp, ch.SEED)
    rx.sync()
    host = f.download((channels, nsamp, 2), np.float32)
    host = host.reshape(channels, blocks, spec.block, 2)
    host *= env[:, :, None, None]
    host = host.reshape(channels, nsamp, 2)
    if q15:
        f.free()
        f = sr.DeviceBuffer(channels * nsamp * 4)
        f.upload((host * 32768.0).astype(np.int16))
    else:
        f.upload(host)
    return f


def time_call(name, channels, nsamp, iters, q15, on, with_meter):
    """median ms per call in _AUTO"""
    spec = ch.baseline_spec(name, channels, sr.ARITH_AUTO)
    rx = sr.Rx(spec.config())
    if on:
        rx.set_cwdec(**PAR)
    if with_meter:
        rx.set_meter(**METER)
    esz = 2 if q15 else 4
    d_in, d_out = keyed_input(rx, spec, channels, nsamp, q15), sr.DeviceBuffer(channels * (nsamp // spec.decim) * esz)
    rx.time_process_each(d_in.ptr, d_out.ptr, nsamp, 3, q15)
    ms = rx.time_process_each(d_in.ptr, d_out.ptr, nsamp, iters, q15)
    rx.sync()
    counts = None
    if on:
        text, count, unit, key = rx.cwdec()
        counts = dict(characters=int(count.sum()), channels_with_text=int((count > 0).sum()), unit_median_blocks=float(np.median(unit)) / 256.0)
    rx.close()
    d_in.free(); d_out.free()
    return float(np.median(ms)), float(ms.min()), float(ms.max()), counts


def isa_rows():
    pkg = os.path.join(ROOT, "selenite-lite_amd")
    flags = subprocess.run(["make", "-s", "-C", pkg, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    flags = [f for f in flags if f != "--offload-compress"]
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "rx_cwdec.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", "-o", asm,
                        os.path.join(pkg, "csrc", "rx_cwdec.hip")], check=True, capture_output=True)
        text = open(asm).read()

    def label(sym):
        m = re.match(r"^_ZN3srx7k_cwdecILi(\d+)EEE", sym)
        return "k_cwdec<%d>" % int(m.group(1)) if m else None

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
    for k in sorted(kern, key=lambda k: int(re.sub(r"\D", "", k))):
        ins = kern[k]
        count = lambda *pre: sum(i.startswith(pre) for i in ins)  # noqa: E731
        # the correctly rounded division is v_div_scale .. v_div_fixup with fused multiply-adds inside: those belong to the operation
        # (and the compiler's u32 divisions -- the magic constant, m / 3 where it is not a multiplication -- go through v_rcp_iflag_f32 and
        # one v_fma_f32 behind it: integer arithmetic)
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
        row.update({"scratch_instructions": count("scratch_", "buffer_"), "fused_multiply_adds": fma_all - fma_div - fma_int, "fma_inside_division": fma_div,
                    "fma_inside_integer_division": fma_int, "divisions": count("v_div_fixup"), "barriers": count("s_barrier"),
                    "vector_instructions": count("v_"), "scalar_instructions": count("s_"), "lds_instructions": count("ds_"),
                    "bpermutes": count("ds_bpermute_b32"),
                    "global_loads": sorted({i.split()[0] for i in ins if i.startswith("global_load")}),
                    "global_stores": sorted({i.split()[0] for i in ins if i.startswith("global_store")})})
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--config", default="cfg4", help="a baseline configuration of selenite_rx.chain (cfg1 .. cfg4)")
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=4096, help="complex input samples per channel and call")
    ap.add_argument("--slots", default="f32,int16")
    ap.add_argument("--only", default="", help="off: the stage-off rows alone; on: the stage-on rows alone (for a kernel trace)")
    ap.add_argument("--with-meter", action="store_true", help="the level meter (gate = 0) on in every row: k_meter next to k_cwdec in a trace")
    ap.add_argument("--isa", action="store_true", help="ISA resources only (no GPU); also written to profiles/cwdec/isa_cwdec.jsonl")
    args = ap.parse_args()
    if args.isa:
        out = os.path.join(ROOT, "profiles", "cwdec", "isa_cwdec.jsonl")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            for row in isa_rows():
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
        return
    lib = os.environ.get("SELENITE_RX_LIB", "in-tree")
    spec = ch.baseline_spec(args.config, 1)
    audio_bytes = args.channels * (args.samples // spec.decim) * 4              # the un-scaled f32 audio of a call: what k_cwdec reads
    for slots in args.slots.split(","):
        q15 = slots == "int16"
        base = {"config": args.config, "channels": args.channels, "samples": args.samples, "blocks": args.samples // spec.block,
                "n": spec.block // spec.decim, "slots": slots, "meter": bool(args.with_meter), "library": lib, "iters": args.iters}
        off = None
        if args.only != "on":
            off, lo, hi, _ = time_call(args.config, args.channels, args.samples, args.iters, q15, False, args.with_meter)
            print(json.dumps(dict(base, cwdec="off", ms_per_call=round(off, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))), flush=True)
        if args.only == "off":
            continue
        med, lo, hi, counts = time_call(args.config, args.channels, args.samples, args.iters, q15, True, args.with_meter)
        row = dict(base, cwdec="on", ms_per_call=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), audio_bytes=audio_bytes)
        row.update(counts)
        if off is not None:
            row["added_ms"] = round(med - off, 4)
            row["call_over_off"] = round(med / off, 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
