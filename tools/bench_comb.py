#!/usr/bin/env python3
"""tools/bench_comb.py -- what the polyphase combiner (include/selenite_comb.h, k_comb<K, Q, OVS, TOut>) costs at the headline's channel
count: 128 bands x K 512 = 65 536 channel rows, 256 frames per row and call (--frames: another call length; 134 MB of f32 I/Q in; 256 x D wideband samples per band out:
134 MB / oversample as f32, half of that as int16), every supported (P, oversample): ms per call (median of --iters launches, one HIP event
between calls on the object's stream; the call is k_comb and the small k_comb_hist behind it), a device-to-device copy of the call's in + out
bytes (hipMemcpyAsync, timed in the same process), and the channeliser (k_chan + k_chan_hist) at the same geometry -- the same K, P and
oversample, 256 x D samples per band in, 256 outputs per channel -- timed in the same run.  The kernel's own time is the k_comb row of
    rocprofv3 --kernel-trace --stats -- python tools/bench_comb.py --only f32 --iters 5
--isa: no GPU; compiles csrc/comb.hip for gfx950 with the library's flags and reads, per k_comb instantiation, VGPRs (architectural +
accumulation), SGPRs, LDS and scratch from the code object's own metadata, and the fused multiply-adds in the kernel (there must be none).
Writes profiles/comb/isa_comb.jsonl.  One JSON line per row."""
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

BANDS, K, FRAMES = 128, 512, 256
SHAPES = [(4, 1), (8, 1), (12, 1), (16, 1), (4, 2), (8, 2)]


def timed(hip, st, run, iters):
    """median, min, max ms of `iters` calls of run() on stream st, one HIP event between calls"""
    vp = C.c_void_p
    ev = [vp() for _ in range(iters + 1)]
    for e in ev:
        if hip.hipEventCreate(C.byref(e)):
            raise RuntimeError("hipEventCreate")
    for _ in range(3):
        run()
    hip.hipEventRecord(ev[0], st)
    for i in range(iters):
        run()
        hip.hipEventRecord(ev[i + 1], st)
    hip.hipEventSynchronize(ev[iters])
    ms = []
    for i in range(iters):
        t = C.c_float()
        hip.hipEventElapsedTime(C.byref(t), ev[i], ev[i + 1])
        ms.append(t.value)
    for e in ev:
        hip.hipEventDestroy(e)
    ms = np.array(ms)
    return float(np.median(ms)), float(ms.min()), float(ms.max())


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
    d = K // ovs
    cb = sr.Combiner(BANDS, K, ovs, p, sr.design_comb_prototype(K, p, 1.0, ovs))
    cb.set_stream(st)
    n = cb.out_len(FRAMES)
    in_bytes, out_bytes = cb.in_channels() * FRAMES * 8, BANDS * n * (4 if q15 else 8)
    rng = np.random.default_rng(7)
    one = rng.uniform(-0.5, 0.5, (K, FRAMES, 2)).astype(np.float32) / np.float32(np.sqrt(K))
    x = np.stack([np.roll(one, 97 * b, axis=1) for b in range(BANDS)])
    d_in, d_out = sr.DeviceBuffer(in_bytes), sr.DeviceBuffer(BANDS * n * 8)
    d_in.upload(x)
    run = cb.process_q15_device if q15 else cb.process_device
    med, lo, hi = timed(hip, st, lambda: run(d_in.ptr, d_out.ptr, FRAMES), iters)
    cb.sync()
    y = d_out.download((BANDS, n, 2), np.int16 if q15 else np.float32)
    assert (q15 or np.isfinite(y).all()) and np.abs(y.astype(np.float64)).max() > 0
    hist_bytes = cb.in_channels() * cb.hist_len * 8
    cb.close()
    # the channeliser the other way: the wideband f32 streams in d_out's place, the channel rows in d_in's
    chz = sr.Channelizer(BANDS, K, ovs, p, sr.design_chan_prototype(K, p, float(ovs)))
    chz.set_stream(st)
    assert chz.out_len(FRAMES * d) == FRAMES
    d_w = sr.DeviceBuffer(BANDS * FRAMES * d * 8)
    d_w.upload(np.ascontiguousarray(x.reshape(-1)[:BANDS * FRAMES * d * 2]))
    cmed, _, _ = timed(hip, st, lambda: chz.process_device(d_w.ptr, d_in.ptr, FRAMES * d), iters)
    chz.sync()
    chz.close()
    hip.hipStreamDestroy(st)
    for b in (d_in, d_out, d_w):
        b.free()
    return med, lo, hi, in_bytes, out_bytes, hist_bytes, cmed


def isa_rows():
    pkg = os.path.join(ROOT, "selenite-lite_amd")
    flags = subprocess.run(["make", "-s", "-C", pkg, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    flags = [f for f in flags if f != "--offload-compress"]
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "comb.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", "-o", asm,
                        os.path.join(pkg, "csrc", "comb.hip")], check=True, capture_output=True)
        text = open(asm).read()

    def label(sym):
        m = re.match(r"^_ZN3srx\S*6k_combILi(\d+)ELi(\d+)ELi(\d+)E([fs])EE", sym)
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
        elif t and not t.startswith(".") and not t.endswith(":"):
            kern[cur].append(t)
    meta = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(_ZN3srx\S+)", blk)
        if not name or not label(name.group(1)):
            continue
        num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))  # noqa: E731
        meta[label(name.group(1))] = dict(vgpr_count=num("vgpr_count"), agpr_count=int(re.match(r"\s*(\d+)", blk).group(1)),
                                          sgpr_count=num("sgpr_count"), lds_bytes=num("group_segment_fixed_size"),
                                          scratch_bytes=num("private_segment_fixed_size"))
    rows = []
    for key in sorted(kern):
        k, q, ovs, t = key
        ins = kern[key]
        count = lambda *pre: sum(i.startswith(pre) for i in ins)  # noqa: E731
        row = {"kernel": "k_comb<%d, %d, %d, %s>" % (k, q, ovs, "float" if t == "f" else "int16_t"), "taps_per_branch": q // ovs}
        row.update(meta.get(key, {}))
        row.update({"scratch_instructions": count("scratch_", "buffer_"),
                    "fused_multiply_adds": sum(bool(re.match(r"v_(pk_)?(fma|fmac|mad|mac)(_mix|_legacy)?_f(16|32|64)", i)) for i in ins),
                    "barriers": count("s_barrier"),
                    "global_loads": sorted({i.split()[0] for i in ins if i.startswith("global_load")}),
                    "global_stores": sorted({i.split()[0] for i in ins if i.startswith("global_store")})})
        rows.append(row)
    return rows


def main():
    global FRAMES
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default="", help="f32: the f32 rows alone (for a kernel trace)")
    ap.add_argument("--frames", type=int, default=FRAMES, help="frames per row and call (default 256)")
    ap.add_argument("--isa", action="store_true", help="ISA resources only (no GPU); also written to profiles/comb/isa_comb.jsonl")
    args = ap.parse_args()
    if args.isa:
        out = os.path.join(ROOT, "profiles", "comb", "isa_comb.jsonl")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            for row in isa_rows():
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
        return
    from bench_meter import copy_ms
    FRAMES = args.frames
    copies = {}
    for q15 in ((False,) if args.only == "f32" else (False, True)):
        for p, ovs in SHAPES:
            med, lo, hi, nin, nout, nhist, cmed = time_call(p, ovs, q15, args.iters)
            total = nin + nout
            if total not in copies:
                copies[total] = copy_ms(total, args.iters)
            row = {"output": "int16" if q15 else "f32", "bands": BANDS, "fft_len": K, "oversample": ovs, "taps_per_branch": p,
                   "frames": FRAMES, "channels": BANDS * K, "ms_per_call": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                   "in_bytes": nin, "out_bytes": nout, "history_bytes_read_and_written": nhist,
                   "GBps_in_plus_out": round(total / med / 1e6, 1),
                   "d2d_copy_of_in_plus_out_ms": round(copies[total], 4), "call_over_copy": round(med / copies[total], 2),
                   "k_chan_f32_same_geometry_ms": round(cmed, 4), "call_over_k_chan": round(med / cmed, 2),
                   "lib": os.path.basename(os.environ.get("SELENITE_RX_LIB", "")), "iters": args.iters}
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
