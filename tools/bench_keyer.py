#!/usr/bin/env python3
"""tools/bench_keyer.py -- what the keyer stage (selenite_tx_set_keyer, csrc/tx_keyer.hip) costs at the TX stages' size: C channels x B
audio samples per call (16 384 x 1024) at the BASELINE-like shape of tools/bench_txcw.py (DSP block 64, L = 4, 256-tap interpolator,
per-channel carriers, a 64-tap keying shape), per-channel units of 12 to 40 WPM at 12 kHz of audio.  Everything in one process, each with
its C-ABI timer (HIP events around `iters` launches on the instance's stream), the variants alternating `rounds` times, medians reported:
  the stage alone, text keying (NULL paddles, every channel sending from its text memory)       -- k_tx_keyer
  the stage alone, random paddles (IAMBIC_B, presses of 1 to 5 units, idle 40 % of the time)    -- k_tx_keyer
  selenite_tx_time_process_key_device on the bytes the stage generated, sidetone off            -- k_tx_cw, the call the stage sits in front of
The stage moves 2 bytes per sample against the modulator's 8 L.  Prints one JSON line.  (profiles/keyer/bench_keyer_shapes.jsonl is this
tool's line from the build that still carried the other kernel shape, one lane per channel, behind the stage timer: the `_lane` rows.)
--isa: no GPU; compiles csrc/tx_keyer.hip for gfx950 with the library's flags and reads, per kernel, VGPRs, SGPRs, LDS and scratch from the
code object's own metadata and counts barriers and scalar / vector / LDS instructions; writes profiles/keyer/isa_keyer.jsonl."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selenite-lite_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = {"10k_tx_keyerE": "k_tx_keyer", "12k_keyer_sendE": "k_keyer_send"}


def isa_rows():
    pkg = os.path.join(ROOT, "selenite-lite_amd")
    flags = subprocess.run(["make", "-s", "-C", pkg, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    flags = [f for f in flags if f != "--offload-compress"]
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "tx_keyer.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", "-o", asm,
                        os.path.join(pkg, "csrc", "tx_keyer.hip")], check=True, capture_output=True)
        text = open(asm).read()

    def label(sym):
        return next((v for k, v in KERNELS.items() if k in sym), None)

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
    for k in ("k_tx_keyer", "k_keyer_send"):
        ins = kern[k]
        count = lambda *pre: sum(i.startswith(pre) for i in ins)  # noqa: E731
        row = {"kernel": k}
        row.update(meta[k])
        row.update({"scratch_instructions": count("scratch_", "buffer_"), "barriers": count("s_barrier"), "vector_instructions": count("v_"),
                    "scalar_instructions": count("s_"), "lds_instructions": count("ds_"), "sgpr_to_lane_moves": count("v_writelane", "v_readlane"),
                    "global_loads": sorted({i.split()[0] for i in ins if i.startswith("global_load")}),
                    "scalar_loads": sorted({i.split()[0] for i in ins if i.startswith("s_load")}),
                    "global_stores": sorted({i.split()[0] for i in ins if i.startswith("global_store")})})
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=16384)
    ap.add_argument("--block-size", type=int, default=1024, help="audio samples per channel and call")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--isa", action="store_true", help="ISA resources only (no GPU); also written to profiles/keyer/isa_keyer.jsonl")
    a = ap.parse_args()
    if a.isa:
        out = os.path.join(ROOT, "profiles", "keyer", "isa_keyer.jsonl")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            for row in isa_rows():
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
        return
    import numpy as np
    import rxcommon as rc
    import selenite_rx as sr
    import txkeyer_oracle as ko

    C_, B = a.channels, a.block_size
    steps = (np.arange(C_, dtype=np.uint64) * 0x00131313 + 0x00800000).astype(np.uint32)       # per-channel carriers, as tools/bench_txcw.py
    spec = rc.TxSpec(C_, nco_steps=steps, mode=rc.MODE_CW)
    L = spec.interp
    units = np.array([sr.keyer_unit(w, 12000.0) for w in np.linspace(12.0, 40.0, C_)], np.uint32)
    rng = np.random.default_rng(rc.SEED)
    units = units[rng.permutation(C_)]                      # every speed in every wave

    def instance(mode):
        tx = sr.Tx(spec.config())
        assert tx.set_cw(sr.keyshape(64), 0.9, sr.tone_step(700.0, 12000.0 * L), 0.25, sr.tone_step(700.0, 12000.0), 0, 5) == 0
        if tx.set_keyer(mode, units, 1024):
            raise SystemExit("the library has no keyer stage")
        return tx

    text_tx, pad_tx = instance(sr.KEYER_IAMBIC_A), instance(sr.KEYER_IAMBIC_B)
    assert text_tx.keyer_send("PARIS " * 170) == 0          # 1020 characters a channel: more than every timed launch together consumes
    pads = ko.random_paddles(rng, 512, B, units[:512], bits=3)
    pads = np.ascontiguousarray(np.tile(pads, (C_ // 512 + 1, 1))[:C_])
    d_pad, d_iq = sr.DeviceBuffer(C_ * B), sr.DeviceBuffer(C_ * B * L * 8)
    d_pad.upload(pads)

    def keyed_on_generated(it):                             # the stage's bytes of the launch before, then the keyed call on them
        text_tx.time_keyer_stage(None, B, 1)
        return text_tx.time_process_key(text_tx.keyer_key_device(), d_iq.ptr, None, B, it)

    runs = {
        "stage_text": lambda it: text_tx.time_keyer_stage(None, B, it),
        "stage_paddles": lambda it: pad_tx.time_keyer_stage(d_pad.ptr, B, it),
        "keyed_call_on_generated_bytes": keyed_on_generated,
    }
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:                   # steady-state clocks
        for f in runs.values():
            f(2)
    t = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, f in runs.items():
            t[k].append(f(a.iters))
    med = {k: float(np.median(v)) for k, v in t.items()}
    key = np.zeros((C_, B), np.uint8)
    assert sr.lib().selenite_rx_memcpy_d2h(key.ctypes.data, text_tx.keyer_key_device(), key.nbytes) == 0
    res = {"metric": "keyer stage alone beside the keyed call on its bytes, ms per launch"}
    res.update({k + "_ms": round(v, 4) for k, v in med.items()})
    res.update({k + "_ms_runs": [round(x, 4) for x in v] for k, v in t.items()})
    res.update({"stage_text_over_keyed_call": round(med["stage_text"] / med["keyed_call_on_generated_bytes"], 4),
                "stage_paddles_over_keyed_call": round(med["stage_paddles"] / med["keyed_call_on_generated_bytes"], 4),
                "stage_bytes": 2 * C_ * B, "keyed_call_bytes": C_ * B * (1 + 8 * L),
                "stage_paddles_fraction_of_8TBps": round(2 * C_ * B / (med["stage_paddles"] * 1e-3) / 8e12, 4),
                "text_pending_min": int(text_tx.keyer_pending().min()), "generated_key_duty": round(float(key.mean()), 4),
                "paddle_duty": round(float((pads != 0).mean()), 4), "channels": C_, "audio_samples_per_call": B, "interp": L,
                "unit_min": int(units.min()), "unit_max": int(units.max()), "iters": a.iters, "rounds": a.rounds})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
