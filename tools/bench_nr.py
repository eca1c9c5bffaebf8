#!/usr/bin/env python3
"""tools/bench_nr.py -- what the NLMS stage (selenite_rx_set_nr) costs at full size: cfg3 and cfg4 (65 536 channels x 4096 samples, _AUTO)
with the stage off and with DENOISE at N = 16 / 32 / 64 (D = 16): ms per call (median of --iters launches, one event between calls) and
the stage's added ms (k_nlms and the AGC pass behind it), and that time as cycles per audio sample and wave at --clock GHz (one wave per 64
channels over the 1024 SIMDs): `cycles_per_sample_at_clock` with the clock it assumed -- give it the clock a counter run measured.
--isa: no GPU; compiles csrc/rx_nlms.hip for gfx950 with the library's flags and reads, per k_nlms<N>, the VGPR / AGPR use and the vector
instructions per audio sample of the unrolled step (the basic block with the most correctly rounded divisions, one per sample), and the
issue floor that count gives at 4 cycles per wave64 vector instruction.  One JSON line per row."""
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


def time_call(name, nr_taps, iters, channels, nsamp):
    spec = ch.baseline_spec(name, channels, sr.ARITH_AUTO)
    rx = sr.Rx(spec.config())
    if nr_taps:
        rx.set_nr(sr.NR_DENOISE, num_taps=nr_taps, delay=16, mu=0.05)
    nout = nsamp // spec.decim
    d_in, d_out = sr.DeviceBuffer(channels * nsamp * 8), sr.DeviceBuffer(channels * nout * 4)
    rx.synth_device(d_in.ptr, 0, channels, 0, nsamp, ch.SEED)
    rx.time_process_each(d_in.ptr, d_out.ptr, nsamp, 3)
    ms = rx.time_process_each(d_in.ptr, d_out.ptr, nsamp, iters)
    rx.sync()
    rx.close()
    return float(np.median(ms)), nout


def isa_rows():
    pkg = os.path.join(ROOT, "selenite-lite_amd")
    flags = subprocess.run(["make", "-s", "-C", pkg, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    flags = [f for f in flags if f != "--offload-compress"]
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "rx_nlms.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", "-o", asm,
                        os.path.join(pkg, "csrc", "rx_nlms.hip")], check=True, capture_output=True)
        text = open(asm).read()
    kern, cur, blk = {}, None, None
    for line in text.split("\n"):
        t = line.split(";")[0].strip()
        m = re.match(r"^_ZN3srx6k_nlmsILi(\d+)E\S*:$", t)
        if m:
            cur = int(m.group(1)); blk = []; kern[cur] = {"blocks": [blk], "all": []}
            continue
        if cur is None:
            continue
        if t.startswith("s_endpgm"):
            cur = None
        elif t.endswith(":"):
            blk = []; kern[cur]["blocks"].append(blk)
        elif t and not t.startswith("."):
            blk.append(t); kern[cur]["all"].append(t)
    meta = {}
    for m in re.finditer(r"\.name:\s+_ZN3srx6k_nlmsILi(\d+)E\S*\n(.*?)\.vgpr_count:\s+(\d+)", text, re.S):
        agpr = re.search(r"\.agpr_count:\s+(\d+)", m.group(2))
        meta[int(m.group(1))] = (int(m.group(3)), int(agpr.group(1)) if agpr else 0)
    rows = []
    for n, k in sorted(kern.items()):
        body = max(k["blocks"], key=lambda b: sum("v_div_fixup_f32" in i for i in b))
        steps = sum("v_div_fixup_f32" in i for i in body)
        vec = [i for i in body if i.startswith(("v_", "ds_", "global_", "buffer_"))]
        rows.append({"kernel": "k_nlms<%d>" % n, "vgpr_count": meta.get(n, (None, None))[0],      # (the metadata's count: VGPRs + AGPRs)
                     "accvgpr_instructions": sum("accvgpr" in i for i in k["all"]),
                     "unrolled_samples": steps, "vector_instructions_per_sample": round(len(vec) / steps, 1),
                     "packed_per_sample": round(sum(i.startswith("v_pk_") for i in body) / steps, 1),
                     "moves_per_sample": round(sum(i.startswith(("v_mov", "v_accvgpr")) for i in body) / steps, 1),
                     "estimate_2.5N+20": 2.5 * n + 20, "issue_floor_cycles_per_sample": round(4 * len(vec) / steps, 1)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--clock", type=float, default=2.1, help="GHz the cycle figure assumes")
    ap.add_argument("--configs", default="cfg3,cfg4")
    ap.add_argument("--taps", default="16,32,64")
    ap.add_argument("--isa", action="store_true", help="ISA counts only (no GPU)")
    args = ap.parse_args()
    if args.isa:
        for row in isa_rows():
            print(json.dumps(row), flush=True)
        return
    for name in args.configs.split(","):
        off, nout = time_call(name, 0, args.iters, args.channels, args.samples)
        print(json.dumps({"config": name, "nr": "off", "ms_per_call": round(off, 4)}), flush=True)
        for n in [int(t) for t in args.taps.split(",")]:
            on, _ = time_call(name, n, args.iters, args.channels, args.samples)
            row = {"config": name, "nr": "denoise", "num_taps": n, "delay": 16, "ms_per_call": round(on, 4), "stage_added_ms": round(on - off, 4),
                   "audio_samples_per_channel": nout}
            # issue floor of the recurrence: one wave per 64 channels, the waves spread over 4 SIMDs x 256 CUs
            waves_per_simd = -(-args.channels // 64) / 1024.0
            row["clock_ghz"] = args.clock
            row["cycles_per_sample_at_clock"] = round((on - off) * 1e-3 * args.clock * 1e9 / (nout * waves_per_simd), 1)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
