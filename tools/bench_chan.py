#!/usr/bin/env python3
"""tools/bench_chan.py -- what the polyphase channeliser (include/selenite_chan.h, k_chan<K, P, OVS, TIn>) costs at the headline's channel
count: 128 bands x K 512 = 65 536 channels, 131 072 wideband samples per band and call (134 MB of f32 I/Q in; 256 x oversample outputs per
channel, 134 MB x oversample out), f32 and int16 input, P 8 and 16, oversample 1 and 2: ms per call (median of --iters launches, one HIP
event between calls on the object's stream; the call is k_chan and the small k_chan_hist behind it), the bytes the call reads and writes, and
two device-to-device copies (hipMemcpyAsync, timed in the same process): one that MOVES the call's bytes (it copies (in + out) / 2 bytes: reads
that many and writes that many) and one that copies in + out bytes (twice the traffic).  The kernel's own time is the k_chan row of
    rocprofv3 --kernel-trace --stats -- python tools/bench_chan.py --only f32 --iters 5
--isa: no GPU; compiles csrc/chan.hip for gfx950 with the library's flags and reads, per k_chan instantiation, VGPRs, SGPRs, LDS and scratch
from the code object's own metadata, the fused multiply-adds in the kernel (there must be none) and the vector, LDS and global instructions
of the innermost loop over a tile's outputs (static counts; with oversample 1 that is one output's straight-line step; with oversample 2 the
two step forms -- the window ends on a multiple of K, or K / 2 past one -- are laid out by the compiler as it sees fit, so those rows are a
lower bound per output: the executed count is a counter run's SQ_INSTS_VALU / outputs).  Writes profiles/chan/isa_chan.jsonl.
One JSON line per row."""
import argparse
import ctypes as C
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

BANDS, K, BLOCK = 128, 512, 131072


def time_call(p, ovs, q15, iters):
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    vp = C.c_void_p
    hip.hipStreamCreate.argtypes = [C.POINTER(vp)]
    hip.hipStreamDestroy.argtypes = [vp]
    hip.hipEventCreate.argtypes = [C.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    hip.hipEventDestroy.argtypes = [vp]
    st = vp()
    if hip.hipStreamCreate(C.byref(st)):
        raise RuntimeError("hipStreamCreate")
    chz = sr.Channelizer(BANDS, K, ovs, p, sr.design_chan_prototype(K, p, float(ovs)))
    chz.set_stream(st)
    nout = chz.out_len(BLOCK)
    in_bytes, out_bytes = BANDS * BLOCK * (4 if q15 else 8), chz.out_channels() * nout * 8
    rng = np.random.default_rng(7)
    one = rng.uniform(-0.5, 0.5, (BLOCK, 2)).astype(np.float32)
    x = np.stack([np.roll(one, 97 * b, axis=0) for b in range(BANDS)])
    d_in, d_out = sr.DeviceBuffer(in_bytes), sr.DeviceBuffer(out_bytes)
    d_in.upload((x * 32768.0).astype(np.int16) if q15 else x)
    run = chz.process_q15_device if q15 else chz.process_device
    ev = [vp() for _ in range(iters + 1)]
    for e in ev:
        if hip.hipEventCreate(C.byref(e)):
            raise RuntimeError("hipEventCreate")
    for _ in range(3):
        run(d_in.ptr, d_out.ptr, BLOCK)
    hip.hipEventRecord(ev[0], st)
    for i in range(iters):
        run(d_in.ptr, d_out.ptr, BLOCK)
        hip.hipEventRecord(ev[i + 1], st)
    hip.hipEventSynchronize(ev[iters])
    chz.sync()
    ms = []
    for i in range(iters):
        t = C.c_float()
        hip.hipEventElapsedTime(C.byref(t), ev[i], ev[i + 1])
        ms.append(t.value)
    for e in ev:
        hip.hipEventDestroy(e)
    y = d_out.download((chz.out_channels(), nout, 2), np.float32)
    assert np.isfinite(y).all() and np.abs(y).max() > 0
    hist_bytes = BANDS * chz.hist_len * 8
    chz.close()
    hip.hipStreamDestroy(st)
    d_in.free(); d_out.free()
    ms = np.array(ms)
    return float(np.median(ms)), float(ms.min()), float(ms.max()), in_bytes, out_bytes, hist_bytes


def isa_rows():
    pkg = os.path.join(ROOT, "selenite-lite_amd")
    flags = subprocess.run(["make", "-s", "-C", pkg, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    flags = [f for f in flags if f != "--offload-compress"]
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "chan.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", "-o", asm,
                        os.path.join(pkg, "csrc", "chan.hip")], check=True, capture_output=True)
        text = open(asm).read()

    def label(sym):
        m = re.match(r"^_ZN3srx\S*6k_chanILi(\d+)ELi(\d+)ELi(\d+)E([fs])EE", sym)
        return (int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4)) if m else None

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

    def output_loop(lines):
        """the loop over a tile's outputs: from a label to the branch back to it, the innermost span (no other loop inside) with the most
        vector instructions"""
        at = {t[:-1]: i for i, t in enumerate(lines) if t.endswith(":")}
        spans = []
        for i, t in enumerate(lines):
            m = re.match(r"s_c?branch\S*\s+(\.LBB\S+)", t)
            if m and m.group(1) in at and at[m.group(1)] < i:
                spans.append((at[m.group(1)], i))
        best = None
        for lo, hi in spans:
            if any((a, b) != (lo, hi) and lo <= a and b <= hi for a, b in spans):
                continue
            body = [x for x in lines[lo:hi + 1] if not x.endswith(":")]
            if best is None or sum(x.startswith("v_") for x in body) > sum(x.startswith("v_") for x in best):
                best = body
        return best

    rows = []
    for key in sorted(kern):
        k, p, ovs, t = key
        ins = [x for x in kern[key] if not x.endswith(":")]
        count = lambda src, *pre: sum(i.startswith(pre) for i in src)  # noqa: E731
        loop = output_loop(kern[key]) or []
        forms = 1.0          # (static counts of the loop as it stands: with oversample 2 the compiler lays the two step forms out its own way)
        row = {"kernel": "k_chan<%d, %d, %d, %s>" % (k, p, ovs, "float" if t == "f" else "int16_t")}
        row.update(meta.get(key, {}))
        row.update({"scratch_instructions": count(ins, "scratch_", "buffer_"),
                    "fused_multiply_adds": sum(bool(re.match(r"v_(pk_)?(fma|fmac|mad|mac)(_mix|_legacy)?_f(16|32|64)", i)) for i in ins),
                    "barriers": count(ins, "s_barrier"),
                    "output_vector_instructions": count(loop, "v_") / forms,
                    "output_f32_add_sub_mul": (count(loop, "v_add_f32", "v_sub_f32", "v_mul_f32") + 2 * count(loop, "v_pk_add_f32", "v_pk_mul_f32")) / forms,
                    "output_register_moves": count(loop, "v_mov_b32", "v_accvgpr", "v_pk_mov_b32") / forms,
                    "output_lds_instructions": count(loop, "ds_") / forms,
                    "output_global_loads": count(loop, "global_load") / forms,
                    "multiply_adds_per_output_per_lane_2PK_over_64": 2 * p * k / 64,
                    "global_stores": sorted({i.split()[0] for i in ins if i.startswith("global_store")})})
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default="", help="f32: the f32 rows alone (for a kernel trace)")
    ap.add_argument("--isa", action="store_true", help="ISA resources only (no GPU); also written to profiles/chan/isa_chan.jsonl")
    args = ap.parse_args()
    if args.isa:
        out = os.path.join(ROOT, "profiles", "chan", "isa_chan.jsonl")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            for row in isa_rows():
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
        return
    from bench_meter import copy_ms
    copies = {}
    for q15 in ((False,) if args.only == "f32" else (False, True)):
        for ovs in (1, 2):
            for p in (8, 16):
                med, lo, hi, nin, nout, nhist = time_call(p, ovs, q15, args.iters)
                total = nin + nout
                for n in (total // 2, total):
                    if n not in copies:
                        copies[n] = copy_ms(n, args.iters)
                row = {"input": "int16" if q15 else "f32", "bands": BANDS, "fft_len": K, "oversample": ovs, "taps_per_branch": p,
                       "block_size": BLOCK, "channels": BANDS * K, "ms_per_call": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                       "in_bytes": nin, "out_bytes": nout, "history_bytes_read_and_written": nhist,
                       "GBps_in_plus_out": round(total / med / 1e6, 1),
                       "d2d_copy_moving_in_plus_out_ms": round(copies[total // 2], 4), "call_over_that_copy": round(med / copies[total // 2], 2),
                       "d2d_copy_of_in_plus_out_ms": round(copies[total], 4), "call_over_this_copy": round(med / copies[total], 2),
                       "iters": args.iters}
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
