#!/usr/bin/env python3
"""tools/output_hashes.py -- SHA-256 of the audio and of the streaming state the library (SELENITE_RX_LIB, else the product) produces for a fixed set
of shapes, arithmetics and slot formats on seeded input: run it with two builds and diff the output to show that a kernel change that was
not meant to change a bit did not (`SELENITE_RX_LIB=old.so python3 tools/output_hashes.py > a; python3 tools/output_hashes.py > b; diff a b`).
The stage rows behind them (NLMS, output stage, spectrum tap: each alone and all three, f32 and int16 slots, device calls and host-pointer
calls cut into 1 MiB channel chunks) hash the audio, the chain state and the stages' state; they run in a child process, because the library
reads SELENITE_RX_HOST_CHUNK_MB once."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selenite-lite_amd"))
import numpy as np  # noqa: E402
import selenite_rx as sr  # noqa: E402
from selenite_rx import chain as ch  # noqa: E402


def stage_rows():
    """cfg3 in SELENITE_ARITH_AUTO, 300 channels with an NCO step each (most of them rerun exactly), three calls of 2048 samples"""
    n, bs = 300, 2048
    steps = (np.arange(n, dtype=np.uint64) * 0x9E3779B1 % (1 << 32)).astype(np.uint32)
    interp = sr.design_interp(32, 4, 0.1)
    for stages in ("nr", "out", "spec", "nr+out+spec"):
        for q15 in (False, True):
            for host in (False, True):
                rx = sr.Rx(ch.baseline_spec("cfg3", n, sr.ARITH_AUTO, nco_steps=steps).config())
                if "nr" in stages:
                    rx.set_nr(sr.NR_DENOISE, num_taps=16, delay=8, mu=0.05)
                if "out" in stages:
                    rx.set_out(4, interp, sr.OUT_STEREO)
                if "spec" in stages:
                    rx.set_spectrum(64, 1, 1, 0.25)
                dt = np.int16 if q15 else np.float32
                vals = rx.out_values(bs)
                d_in, d_out = sr.DeviceBuffer(n * bs * 2 * np.dtype(dt).itemsize), sr.DeviceBuffer(n * vals * np.dtype(dt).itemsize)
                h = hashlib.sha256()
                for call in range(3):
                    data = sr.synth_iq_host(0, n, call * bs, bs, ch.SEED)
                    if q15:
                        data = np.clip(np.trunc(data * 32768.0), -32768, 32767).astype(np.int16)
                    if host:
                        y = (rx.process_q15 if q15 else rx.process)(data)
                    else:
                        d_in.upload(data)
                        (rx.process_q15_device if q15 else rx.process_device)(d_in.ptr, d_out.ptr, bs)
                        rx.sync()
                        y = d_out.download((n, vals), dt)
                    h.update(np.ascontiguousarray(y).tobytes())
                state = [rx.state()]
                if "nr" in stages:
                    state.append(rx.nr_state())
                if "out" in stages:
                    state.append(dict(interp=rx.out_state()))
                if "spec" in stages:
                    state.append(rx.spectrum_state())
                for st in state:
                    for k in sorted(st):
                        h.update(np.ascontiguousarray(st[k]).tobytes())
                print("stages", stages, "q15" if q15 else "f32", "host-chunked" if host else "device", rx.kernel_name(), h.hexdigest()[:24])
                rx.close(); d_in.free(); d_out.free()


SHAPES = [("cfg1", 256 * 4), ("cfg2", 256 * 5), ("cfg2_48k128", 128 * 7), ("cfg2_48k", 192 * 5), ("cfg3", 1024 * 3), ("cfg3_by8", 2048), ("cfg4", 256 * 4)]


def chain_rows():
    for name, bs in SHAPES:
        for arith in (sr.ARITH_CMSIS, sr.ARITH_FMA, sr.ARITH_SPLIT16, sr.ARITH_AUTO):
            for q15 in (False, True):
                for mode in (sr.MODE_USB, sr.MODE_LSB, sr.MODE_AM):
                    if name == "cfg4" and mode != sr.MODE_USB:
                        continue
                    n = 96
                    spec = ch.baseline_spec(name, n, arith)
                    if name != "cfg4":
                        spec.mode = mode
                    rx = sr.Rx(spec.config())
                    h = hashlib.sha256()
                    for call in range(3):
                        iq = sr.synth_iq_host(0, n, call * bs, bs, ch.SEED)
                        if q15:
                            y = rx.process_q15(np.clip(np.trunc(iq * 32768.0), -32768, 32767).astype(np.int16))
                        else:
                            y = rx.process(iq)
                        h.update(np.ascontiguousarray(y).tobytes())
                    st = rx.state()
                    for k in sorted(st):
                        h.update(np.ascontiguousarray(st[k]).tobytes())
                    print(name, arith, "q15" if q15 else "f32", mode, rx.kernel_name(), h.hexdigest()[:24])
                    rx.close()


def main():
    if sys.argv[1:] == ["--stage-rows"]:
        stage_rows()
        return 0
    chain_rows()
    sys.stdout.flush()
    # a fresh child process: the library reads SELENITE_RX_HOST_CHUNK_MB once
    return subprocess.run([sys.executable, os.path.abspath(__file__), "--stage-rows"], env=dict(os.environ, SELENITE_RX_HOST_CHUNK_MB="1")).returncode


if __name__ == "__main__":
    sys.exit(main())
