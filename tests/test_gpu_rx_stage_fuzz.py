"""GPU: random subsets of the nine RX stages, random chains and random call sequences against ONE composed oracle (tests/rx_pipeline_oracle.py:
Pipeline, the per-stage restatements in the order of DESIGN.md section 2) -- the executor behind csrc/rx_route.h (rx_dispatch.hip: run_front,
run_part, with_out_stage) held to an independent statement of what every combination must return and leave behind.

tests/rx_stage_fuzz_cases.py draws the cases (tests/test_rx_stage_fuzz_cases.py asserts on the CPU what they reach): four chain families, the
six modes, the NCO flavours, the four arithmetics, the AGC off / per channel / global, 1 .. 70 channels, each stage on with probability 1/2
with parameters away from their defaults, and 3 .. 7 events: calls of 1 .. 20 DSP blocks through the four entries, the global gain in one
call and split in its two phases (a state read in between), set_mode, reset, checkpoint / restore into a fresh instance, a stage removed
and a stage set mid-stream, and the split call refused on an instance with an output stage.

Behind EVERY event, on bits: the returned audio or frames; the chain state; every row of every enabled stage's state; the spectrum's frame
count.  SELENITE_ARITH_CMSIS / _FMA: the oracle chain is the audio source.  _SPLIT16 / _AUTO: the chain is tolerance-based by construction
(tests/test_gpu_fuzz.py, tests/test_gpu_auto.py hold it to its bar), so the un-scaled audio is that of a twin instance with the same chain,
I/Q correction and blanker, its AGC off and nothing behind the chain (the method of tests/test_gpu_cwdec.py: Tap) and everything behind
the chain is still compared on bits; the chain state is the twin's, the AGC gain the oracle's.

A failure names the case and the event: SELENITE_RX_STAGE_FUZZ_ONLY=<index> runs that case of a family alone;
SELENITE_RX_STAGE_FUZZ_CASES=<n> scales the counts (rx_stage_fuzz_cases.COUNTS)."""
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rx_stage_fuzz_cases as fz
import rxcommon as rc
import selenite_rx as sr

pytestmark = pytest.mark.gpu

GETTERS = dict(spectrum="spectrum_state", iqc="iqc_state", nb="nb_state", tones="tones_state", cwdec="cwdec_state", afilt="afilt_state",
               nr="nr_state", meter="meter_state", out="out_state")
KERNEL = dict(ssb_fused=("k_ssb_", "k_hilb_"), cw_fused=("k_cw_fused",), generic=("generic",))


def set_stage(rx, name, p):
    """Rx.set_<name> with the case's parameters, or with None the stage's removal"""
    if name == "tones":
        rx.set_tones(None if p is None else np.array(p["coeffs"], np.float32), **({} if p is None else {k: v for k, v in p.items() if k != "coeffs"}))
    elif name == "afilt":
        rx.set_afilt(None) if p is None else rx.set_afilt(np.array(p["coeffs"], np.float32), p["per_channel"])
    elif name == "nr":
        rx.set_nr(sr.NR_OFF) if p is None else rx.set_nr(**p)
    elif name == "meter":
        rx.set_meter(sense=None) if p is None else rx.set_meter(**p)
    elif name == "out":
        rx.set_out(None) if p is None else rx.set_out(p["interp"], p["coeffs"], p["frames"])
    elif name == "cwdec":
        rx.set_cwdec(None) if p is None else rx.set_cwdec(**p)
    elif name == "spectrum":
        rx.set_spectrum(None) if p is None else rx.set_spectrum(**p)
    else:
        getattr(rx, "set_" + name)(None) if p is None else getattr(rx, "set_" + name)(**p)


def make_rx(case, on, mode, twin=False):
    """an instance of the case in `mode` with the stages `on`; twin: AGC off and only what stands in front of the chain"""
    spec = fz.build_spec(case, mode=mode, **(dict(agc=False, agc_global=False) if twin else {}))
    with (sr.plan_option(sr.OPT_FORCE_GENERIC) if case["force_generic"] else contextlib.nullcontext()):
        rx = sr.Rx(spec.config())
    if spec.arith == rc.ARITH_AUTO:
        rx.set_auto_launches(case["auto_launches"])
    for name in on:
        if not twin or name in ("iqc", "nb"):
            set_stage(rx, name, case["params"][name])
    return rx


def has_state(rx, name):
    return name != "out" or rx._out[1] >= 2                      # (an interpolator of one tap per phase keeps no history)


def read_state(rx, on):
    d = {"chain": rx.state()}
    for name in on:
        if has_state(rx, name):
            d[name] = getattr(rx, GETTERS[name])()
    return d


def restore(rx, st):
    rx.set_state(st["chain"])
    for name, rows in st.items():
        if name != "chain":
            getattr(rx, "set_" + GETTERS[name])(rows)


def differing(got, want):
    """None, or where two arrays differ: dtype / shape, or the first differing index with both values"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return "%s %s against %s %s" % (got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() == want.tobytes():
        return None
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.itemsize]
    bad = np.argwhere(np.atleast_1d(got).view(u) != np.atleast_1d(want).view(u))
    at = tuple(int(v) for v in bad[0])
    return "%d of %d values differ, first at %s (row %d): %r against %r" % (len(bad), got.size, list(at), at[0], np.atleast_1d(got)[at].item(),
                                                                           np.atleast_1d(want)[at].item())


def check(got, want, what):
    d = differing(got, want)
    assert d is None, "%s: %s" % (what, d)


def check_states(got, want, what):
    assert set(got) == set(want), "%s: states %s against %s" % (what, sorted(got), sorted(want))
    for name in want:
        if isinstance(want[name], dict):
            assert set(got[name]) == set(want[name]), "%s: %s rows %s against %s" % (what, name, sorted(got[name]), sorted(want[name]))
            for k in want[name]:
                check(got[name][k], want[name][k], "%s: %s state, %s" % (what, name, k))
        else:
            check(got[name], want[name], "%s: %s state" % (what, name))


class Buffers:
    """device buffers of one call"""

    def __init__(self, *sizes):
        self.b = [sr.DeviceBuffer(n) for n in sizes]

    def __enter__(self):
        return self.b

    def __exit__(self, *a):
        for b in self.b:
            b.free()


def call(rx, data, entry):
    """one process call through one of the four entries"""
    q15 = data.dtype == np.int16
    if entry.startswith("host"):
        return rx.process_q15(data) if q15 else rx.process(data)
    ch, bs = data.shape[0], data.shape[1]
    vals = rx.out_len(bs)
    with Buffers(data.nbytes, ch * vals * data.dtype.itemsize) as (d_in, d_out):
        d_in.upload(np.ascontiguousarray(data))
        (rx.process_q15_device if q15 else rx.process_device)(d_in.ptr, d_out.ptr, bs)
        rx.sync()
        return d_out.download((ch, vals), data.dtype)


def one_call(rx, data):
    """selenite_rx_global_process_f32_device with a NULL communicator"""
    ch, bs = data.shape[0], data.shape[1]
    vals = rx.out_len(bs)
    rx.L.selenite_rx_global_process_f32_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    with Buffers(data.nbytes, ch * vals * 4) as (d_in, d_out):
        d_in.upload(np.ascontiguousarray(data))
        assert rx.L.selenite_rx_global_process_f32_device(rx.h, d_in.ptr, d_out.ptr, bs, None) == 0, rx.error()
        rx.sync()
        return d_out.download((ch, vals), np.float32)


class Run:
    """one case on the GPU beside its oracle"""

    def __init__(self, case):
        self.case, self.spec = case, case["spec"]
        self.tol = fz.oracle_arith(case) is None
        self.on, self.mode, self.at = list(case["on"]), self.spec["mode"], 0
        self.p = fz.pipeline_of(case)
        self.rx = make_rx(case, self.on, self.mode)
        self.twin = make_rx(case, self.on, self.mode, twin=True) if self.tol else None
        self.na = self.spec["block"] // self.spec["decim"]
        self.diverged = False

    def oracle_diverged(self):
        """arm_lms_norm_f32 keeps its window's energy as a running difference (energy -= x0 * x0; energy += in * in): behind a large sample the
        float32 residue can be negative, energy + 1.19e-7 then passes zero and the weights overflow -- in the reference, in the oracle and in
        the library alike (which then reports SELENITE_RX_NANINF for good).  Such a call is no comparison of bits: the case ends in front of it."""
        nr = self.p.st.get("nr")
        self.diverged = nr is not None and not (np.isfinite(nr.coeffs).all() and np.isfinite(nr.energy).all())
        return self.diverged

    def what(self, i):
        ev = self.case["events"][i]
        return "%s case %d, event %d (%s): %s" % (self.case["kind"], self.case["idx"], i, ev["op"], json.dumps({k: v for k, v in ev.items() if k != "op"}))

    def close(self):
        self.rx.close()
        if self.twin is not None:
            self.twin.close()

    def pre(self, data):
        """the un-scaled audio of the call where the oracle does not make it itself: the twin's, of the f32 call the int16 call runs as"""
        if not self.tol:
            return None
        return self.twin.process(np.divide(data.astype(np.float32), np.float32(32768.0)) if data.dtype == np.int16 else data)

    def compare_states(self, rx, what):
        got, want = read_state(rx, self.on), self.p.state()
        if self.tol:
            tw = self.twin.state()
            want["chain"].update({k: v for k, v in tw.items() if k != "agc_gain"})
        check_states(got, want, what)
        if "spectrum" in self.on:
            frames = rx.spectrum()[1]
            assert frames == self.p.spectrum_frames(), "%s: %d spectrum frames, not %d" % (what, frames, self.p.spectrum_frames())
        assert rx.status() == 0, "%s: status %d: %s" % (what, rx.status(), rx.error())

    def kernel(self, what):
        fam, name = fz.kernel_family(self.case, self.mode), self.rx.kernel_name()
        assert name.startswith(KERNEL[fam]), "%s: kernel %s, the generator's restatement says %s" % (what, name, fam)

    def checkpoint(self, what):
        """every state into a fresh instance; returns the old one (SELENITE_ARITH_CMSIS / _FMA: both then run the next call)"""
        st = read_state(self.rx, self.on)
        old, self.rx = self.rx, make_rx(self.case, self.on, self.mode)
        restore(self.rx, st)
        check_states(read_state(self.rx, self.on), st, what + ": the restored instance")
        if "spectrum" in self.on:
            assert self.rx.spectrum()[1] == old.spectrum()[1], what + ": the restored frame count"
        q = fz.pipeline_of(self.case, on=self.on, mode=self.mode)
        q.set_state(self.p.state())
        self.p = q
        if self.tol:                                             # (the twin is restored too: both instances then stand behind the same history)
            keep = [k for k in self.on if k in ("iqc", "nb")]
            st = read_state(self.twin, keep)
            self.twin.close()
            self.twin = make_rx(self.case, self.on, self.mode, twin=True)
            restore(self.twin, st)
            old.close()
            return None
        return old

    def event(self, i):
        ev, case, what = self.case["events"][i], self.case, self.what(i)
        op = ev["op"]
        both = (self.rx,) + ((self.twin,) if self.tol else ())
        if op == "set_mode":
            self.mode = ev["mode"]
            for r in both:
                assert r.set_mode(self.mode) == 0, what
            self.p.set_mode(self.mode)
            self.kernel(what)
        elif op == "reset":
            for r in both:
                assert r.reset() == 0, what
            self.p.reset()
        elif op in ("drop_stage", "add_stage"):
            name = ev["stage"]
            par = case["params"][name] if op == "add_stage" else None
            self.on = [k for k in fz.STAGES if (k in self.on and k != name) or (k == name and par is not None)]
            set_stage(self.rx, name, par)
            if self.tol and name in ("iqc", "nb"):
                set_stage(self.twin, name, par)
            self.p.set_stage(name, par)
        elif op == "refused_split":
            bs = ev["blocks"] * self.spec["block"]
            before = read_state(self.rx, self.on)
            with Buffers(self.spec["channels"] * bs * 8, self.spec["channels"] * (bs // self.spec["decim"]) * 4, 4 * ev["blocks"]) as (d_in, d_out, d_env):
                d_in.upload(fz.signal(case, self.at, bs))
                self.rx.global_phase1(d_in.ptr, d_out.ptr, d_env.ptr, bs)
                assert self.rx.status() == sr.ARGUMENT_ERROR and "output stage" in self.rx.error(), what
                self.rx.global_phase2(d_out.ptr, d_env.ptr, bs)
                assert self.rx.status() == sr.ARGUMENT_ERROR, what
            check_states(read_state(self.rx, self.on), before, what + ": the refused call moved")
            return False                                         # (the status is sticky: the case ends here)
        else:
            old = self.checkpoint(what) if op == "checkpoint" else None
            bs = ev["blocks"] * self.spec["block"]
            data = fz.signal(case, self.at, bs)
            self.at += bs
            if ev.get("entry", "").endswith("q15"):
                data = fz.to_q15(data)
            pre = self.pre(data)
            if op == "global_split":
                ch, nout = self.spec["channels"], bs // self.spec["decim"]
                a, env = self.p.phase1(data, pre)
                if self.oracle_diverged():
                    return False
                with Buffers(data.nbytes, ch * nout * 4, 4 * ev["blocks"]) as (d_in, d_out, d_env):
                    d_in.upload(data)
                    self.rx.global_phase1(d_in.ptr, d_out.ptr, d_env.ptr, bs)
                    self.rx.sync()
                    check(d_out.download((ch, nout), np.float32), a, what + ": un-scaled audio behind phase 1")
                    check(d_env.download((ev["blocks"],), np.float32), env, what + ": envelope row of phase 1")
                    self.compare_states(self.rx, what + ": between the phases")
                    self.rx.global_phase2(d_out.ptr, d_env.ptr, bs)
                    self.rx.sync()
                    got = d_out.download((ch, nout), np.float32)
                want = self.p.phase2()
            else:
                want = self.p.process_audio(pre, data)
                if self.oracle_diverged():
                    if old is not None:
                        old.close()
                    return False
                got = one_call(self.rx, data) if op == "global_one_call" else call(self.rx, data, ev["entry"])
                if old is not None:
                    check(call(old, data, ev["entry"]), want, what + ": the instance the checkpoint was read from")
                    self.compare_states(old, what + ": the instance the checkpoint was read from")
                    old.close()
            check(got, want, what + (": frames" if "out" in self.on else ": audio"))
            self.compare_states(self.rx, what)
        return True


def run_case(case):
    r = Run(case)
    try:
        r.kernel(r.what(0))
        r.compare_states(r.rx, "%s case %d, behind the setters" % (case["kind"], case["idx"]))
        for i in range(len(case["events"])):
            try:
                if not r.event(i):
                    break
            except AssertionError:
                raise
            except Exception as e:                               # (a refused setter, a sticky status: name the case and the event as well)
                raise AssertionError("%s: %s: %s" % (r.what(i), type(e).__name__, e)) from e
    finally:
        r.close()
    return r.diverged


def run_slice(kind):
    n = fz.scale_count(kind, os.environ.get("SELENITE_RX_STAGE_FUZZ_CASES"))
    only = os.environ.get("SELENITE_RX_STAGE_FUZZ_ONLY")
    ran, diverged = 0, []
    for case in fz.cases(fz.SEED, n, kind):
        if only is None or case["idx"] == int(only):
            if run_case(case):
                diverged.append(case["idx"])
            ran += 1
    print("rx stage fuzz %s: %d cases; ended early because the NLMS oracle itself overflowed: %s" % (kind, ran, diverged))
    assert not diverged or n > fz.COUNTS[kind], "the default cases are finite throughout: %s" % diverged


def test_ssb_chains():
    run_slice("ssb")


def test_hilbert_pair_chains_without_decimator():
    run_slice("hilb")


def test_cw_chains_on_the_fused_cw_kernel():
    run_slice("cw")


def test_generic_shapes_and_forced_generic_kernels():
    run_slice("generic")


# ---- ragged channel chunks of a host call -------------------------------------------------------------------------------------------------------
def chunk_child():
    """(in a child process, SELENITE_RX_HOST_CHUNK_MB=1) two cases with all nine stages on, 300 channels x 2048 samples, f32 and int16: the
    host-pointer call -- cut by the pipeline into ragged channel chunks -- equals the device-pointer call and the oracle on bits, frames and
    every state"""
    for case in fz.chunk_cases():
        for q15 in (False, True):
            r = Run(case)
            host = make_rx(case, r.on, r.mode)
            what = "chunked %s case %d, %s" % (case["kind"], case["idx"], "int16" if q15 else "f32")
            data = fz.signal(case, 0, 2048)
            if q15:
                data = fz.to_q15(data)
            want = r.p.process_audio(r.pre(data), data)
            check(call(r.rx, data, "dev"), want, what + ": device-pointer call against the oracle")
            check(call(host, data, "host"), want, what + ": host-pointer call against the oracle")
            r.compare_states(r.rx, what + ": device-pointer call")
            r.compare_states(host, what + ": host-pointer call")
            host.close()
            r.close()
    print("OK")


def test_all_nine_stages_across_ragged_channel_chunks():
    env = dict(os.environ, SELENITE_RX_HOST_CHUNK_MB="1")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_rx_stage_fuzz as t; t.chunk_child()" % (os.path.join(rc.ROOT, "tests"), rc.PKG_DIR)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), (out.stdout[-1000:], out.stderr[-3000:])
