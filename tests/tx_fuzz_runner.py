"""One GPU TX instance and its oracle side by side (tests/test_gpu_tx_fuzz.py, tests/test_gpu_tx_edges.py, tests/test_gpu_tx_entry_edges.py):
every operation goes to both, every call is compared -- output, every state array, the status -- as the arithmetic of the instance allows:

    SELENITE_ARITH_CMSIS / _FMA   output and state on bits against txfm_oracle.TxFmOracle of the same arithmetic
    SELENITE_ARITH_SPLIT16        state on bits against the FMA oracle (tests/test_gpu_tx.py: test_tx_split16_interpolator_on_the_matrix_pipe);
                                  output on bits against the FMA oracle wherever k_tx_split16 does not serve the call (FM, k_tx_generic,
                                  a shape without the matrix kernel); a call on k_tx_split16 against the CMSIS oracle, per channel and per
                                  256 complex outputs max|gpu - ref| <= TOL max|ref| (f32; TOL of tests/test_gpu_tx.py), at most 1 LSB (int16)

The CMSIS oracle of a SPLIT16 instance takes both phase accumulators from the FMA oracle behind every call: in FM the phase is the running
sum of the modulation, the two arithmetics round the modulating signal differently, and a reference that starts a later call from another
phase is no reference for it.  Its filter states stay its own, as in the existing split16 tests.

Pair follows an instance with the audio entries alone against txfm_oracle.TxFmOracle.  EntryPair follows one with a keyed CW path and an
audio input stage through all three kinds of entry against txin_oracle.TxInOracle (whose chain is txcw_oracle.TxCwOracle), under the same
arithmetic rules; on top of them it compares the stage's audio (in_audio_device) and the sidetone buffer on bits in every arithmetic, and
cw_state, in_state and fm_state with the chain's.

TEST INFRASTRUCTURE.  Nothing here is imported by the product.
"""
import copy

import numpy as np

import rxcommon as rc
import tx_fuzz_cases as fz
import tx_entry_fuzz_cases as ez
import txfm_oracle as fo
import txin_oracle as tio
from test_gpu_tx import TOL

f32 = np.float32
WORST = [0.0]            # the worst k_tx_split16 per-block error of this process, as a fraction of the block maximum
STATE_KEYS = ("fir_state", "interp_state", "alc_gain", "nco_phase")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def first_difference(got, want):
    u = {2: np.uint16, 4: np.uint32}[got.itemsize]
    bad = np.argwhere(got.view(u) != want.view(u))
    return "%d of %d values differ, first at %s: %r vs %r" % (len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not same_bits(got, want):
        raise AssertionError("%s: %s" % (what, first_difference(got, want)))


def assert_iq(y, want, ref, on_split16, q15, served, what):
    """the I/Q of one call: on bits against `want`, or (a call k_tx_split16 served) at its bar against `ref`, the CMSIS twin's"""
    if not on_split16:
        assert_bits(y, want, "%s output (%s)" % (what, served))
        return
    assert y.shape == ref.shape and y.dtype == ref.dtype
    if q15:
        d = int(np.abs(y.astype(np.int32) - ref.astype(np.int32)).max())
        assert d <= 1, "%s k_tx_split16 int16: %d LSB from the CMSIS arithmetic" % (what, d)
        return
    assert np.isfinite(y).all()
    nch, n = y.shape[0], y.shape[1]
    d = np.abs(y.astype(np.float64) - ref).reshape(nch, n // 256, -1).max(axis=2)
    m = np.abs(ref.astype(np.float64)).reshape(nch, n // 256, -1).max(axis=2)       # (a gated block is all +0.0f: then d must be 0)
    worst = float((d[m > 0] / m[m > 0]).max()) if (m > 0).any() else 0.0
    WORST[0] = max(WORST[0], worst)
    assert (d <= TOL * m).all(), "%s k_tx_split16: a block %.3g of its maximum from the CMSIS arithmetic (bar %g)" % (what, worst, TOL)


class Pair:
    def __init__(self, spec, fm=None, kernel=None):
        """fm: (deviation, amplitude, tone_level, tone_steps) or None; kernel: what kernel_name() must say in the spec's mode"""
        import selenite_rx as sr
        self.sr, self.spec = sr, spec
        self.g = sr.Tx(spec.config())
        if kernel is not None:
            assert self.g.kernel_name() == kernel, (self.g.kernel_name(), kernel)
        self.split = spec.arith == rc.ARITH_SPLIT16
        self.matrix = self.g.kernel_name() == fz.SPLIT16
        exact = spec
        if self.split:
            exact = copy.copy(spec)
            exact.arith = rc.ARITH_FMA
        self.o = fo.TxFmOracle(exact)
        self.oc = None
        if self.matrix:
            plain = copy.copy(spec)
            plain.arith = rc.ARITH_CMSIS
            self.oc = fo.TxFmOracle(plain)
        if fm is not None:
            self.set_fm(*fm)

    def close(self):
        self.g.close()

    def _both(self, name, *args):
        want = getattr(self.o, name)(*args)
        if self.oc is not None:
            assert getattr(self.oc, name)(*args) == want
        return want

    # ---- operations that change no sample ----
    def set_mode(self, mode, kernel=None):
        want = self._both("set_mode", mode)
        before = self.g.kernel_name()
        assert self.g.set_mode(mode) == want, "set_mode(%d): status" % mode
        if want != 0:
            assert want == rc.ARGUMENT_ERROR and self.g.kernel_name() == before, "a refused set_mode keeps the mode"
        if kernel is not None:
            assert self.g.kernel_name() == kernel, "kernel_name %s, expected %s" % (self.g.kernel_name(), kernel)
        return want

    def set_fm(self, deviation, amplitude, tone_level, tone_steps):
        assert self.g.set_fm(deviation, amplitude, tone_level, tone_steps) == 0
        self._both("set_fm", deviation, amplitude, tone_level, tone_steps)

    def clear_fm(self):
        want = self._both("clear_fm")
        assert self.g.clear_fm() == want
        return want

    def reset(self):
        assert self.g.reset() == 0
        self._both("reset")
        self.assert_state("behind reset()")

    def set_phase(self, phase):
        """selenite_tx_set_state with every channel's nco_phase at `phase` (the other arrays as they are)"""
        st = self.g.state()
        st["nco_phase"][:] = phase
        self.g.set_state(st)
        self._both("set_phase", phase)

    # ---- state ----
    def gpu_state(self):
        st = self.g.state()
        if self.o.fm_set:
            st["tone_phase"] = self.g.fm_state()["tone_phase"]
        return st

    def restore(self, st):
        self.g.set_state({k: st[k] for k in STATE_KEYS})
        if "tone_phase" in st:
            self.g.set_fm_state(st)

    def assert_state(self, what=""):
        sg, so = self.gpu_state(), self.o.state()
        if not self.o.fm_set:
            assert not so["tone_phase"].any()
            del so["tone_phase"]
        assert set(sg) == set(so)
        for k in so:
            assert_bits(sg[k], so[k], "state %s %s" % (k, what))

    # ---- calls ----
    def gpu_call(self, x, device=False):
        g, q15 = self.g, x.dtype == np.int16
        if not device:
            y = g.process_q15(x) if q15 else g.process(x)
        else:
            nch, bs = x.shape
            shape = (nch, bs * self.spec.interp, 2)
            d_in, d_out = self.sr.DeviceBuffer(x.nbytes), self.sr.DeviceBuffer(int(np.prod(shape)) * x.itemsize)
            d_in.upload(x)
            (g.L.selenite_tx_process_q15_device if q15 else g.L.selenite_tx_process_f32_device)(g.h, d_in.ptr, d_out.ptr, bs)
            assert g.sync() == 0
            y = d_out.download(shape, x.dtype)
            d_in.free()
            d_out.free()
        assert g.sync() == 0, "sync()"
        g.check()
        return y

    def call(self, x, device=False, served=None, what=""):
        """served: the kernel family that must serve the call, where the caller knows it (fz.walk); None: from the host's rule"""
        q15 = x.dtype == np.int16
        if served is None:
            served = fz.FAMILY[self.g.kernel_name()]
            if served in ("fused", "split16") and x.shape[1] % 256:
                served = "generic"
        y = self.gpu_call(x, device)
        want = self.o.process_q15(x) if q15 else self.o.process(x)
        if self.oc is not None:
            ref = self.oc.process_q15(x) if q15 else self.oc.process(x)
            self.oc.phase[:], self.oc.tone_phase[:] = self.o.phase, self.o.tone_phase
        if self.split and served == "split16":
            assert self.matrix
            assert y.shape == ref.shape and y.dtype == ref.dtype
            if q15:
                d = int(np.abs(y.astype(np.int32) - ref.astype(np.int32)).max())
                assert d <= 1, "%s k_tx_split16 int16: %d LSB from the CMSIS arithmetic" % (what, d)
            else:
                assert np.isfinite(y).all()
                nch, n = y.shape[0], y.shape[1]
                d = np.abs(y.astype(np.float64) - ref).reshape(nch, n // 256, -1).max(axis=2)
                m = np.abs(ref).reshape(nch, n // 256, -1).max(axis=2)
                worst = float((d / np.maximum(m, 1e-300)).max()) if (m > 0).any() else 0.0
                WORST[0] = max(WORST[0], worst)
                assert (d <= TOL * m).all(), "%s k_tx_split16: a block %.3g of its maximum from the CMSIS arithmetic (bar %g)" % (what, worst, TOL)
        else:
            assert_bits(y, want, "%s output (%s)" % (what, served))
        self.assert_state(what)
        return y

    def checkpoint_call(self, x, device=False, served=None, what=""):
        """state() + fm_state(), the call, restore, the same call again: the bits and the state of the first time"""
        snap = self.gpu_state()
        y = self.call(x, device, served, what)
        after = self.gpu_state()
        self.restore(snap)
        again = self.gpu_state()
        for k in snap:
            assert_bits(again[k], snap[k], "%s restored %s" % (what, k))
        assert_bits(self.gpu_call(x, device), y, what + " replay behind the restore")
        again = self.gpu_state()
        for k in after:
            assert_bits(again[k], after[k], "%s state %s behind the replay" % (what, k))
        return y


def run_case(case):
    """Every event of a fz case on a Pair; an assertion carries the whole case and the event index"""
    i, p = -1, None
    try:
        spec = fz.build_spec(case)
        p = Pair(spec, fz.fm_args(case["fm"]) if case["fm"] else None, kernel=fz.expected_kernel(case))
        served = {}
        for ei, rec in fz.walk(case):
            served[ei] = rec["kernel"]
        for i, ev in enumerate(case["events"]):
            op, what = ev["op"], "event %d (%s)" % (i, ev["op"])
            if op == "set_mode":
                assert p.set_mode(ev["mode"], fz.expected_kernel(case, ev["mode"])) == 0
            elif op == "refused_fm":
                assert p.set_mode(fz.FM) == rc.ARGUMENT_ERROR
            elif op == "set_fm":
                p.set_fm(*fz.fm_args(ev["fm"]))
            elif op == "reset":
                p.reset()
            elif op == "set_phase":
                p.set_phase(ev["phase"])
            elif op == "process":
                p.call(fz.audio(case, ev), ev["device"], served[i], what)
            else:
                assert op == "checkpoint"
                p.checkpoint_call(fz.audio(case, ev), ev["device"], served[i], what)
    except AssertionError as e:
        raise AssertionError("%s\n  at event %d of case %r" % (e, i, case)) from e
    finally:
        if p is not None:
            p.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# instances with a keyed CW path and an audio input stage: three kinds of entry on one instance
# ---------------------------------------------------------------------------------------------------------------------------------------
KINDS = {"f32": tio.K_F32, "q15": tio.K_Q15, "q15f": tio.K_Q15_F32}


class EntryPair:
    def __init__(self, spec, kernel=None):
        import selenite_rx as sr
        self.sr, self.spec = sr, spec
        self.g = sr.Tx(spec.config())
        if kernel is not None:
            assert self.g.kernel_name() == kernel, (self.g.kernel_name(), kernel)
        self.split = spec.arith == rc.ARITH_SPLIT16
        self.matrix = self.g.kernel_name() == fz.SPLIT16
        exact = spec
        if self.split:
            exact = copy.copy(spec)
            exact.arith = rc.ARITH_FMA
        self.o = tio.TxInOracle(exact)
        self.oc = None
        if self.matrix:
            plain = copy.copy(spec)
            plain.arith = rc.ARITH_CMSIS
            self.oc = tio.TxInOracle(plain)
        self.fm_set = self.cw_set = self.in_set = False

    def close(self):
        self.g.close()

    def _both(self, chain, name, *args, **kw):
        want = getattr(self.o.chain if chain else self.o, name)(*args, **kw)
        if self.oc is not None:
            assert getattr(self.oc.chain if chain else self.oc, name)(*args, **kw) == want
        return want

    def _rephase(self):
        if self.oc is not None:
            self.oc.chain.phase[:], self.oc.chain.tone_phase[:] = self.o.chain.phase, self.o.chain.tone_phase

    # ---- operations that change no sample ----
    def set_mode(self, mode, kernel=None):
        want = self._both(False, "set_mode", mode)
        before = self.g.kernel_name()
        assert self.g.set_mode(mode) == want, "set_mode(%d): status" % mode
        if want != 0:
            assert want == rc.ARGUMENT_ERROR and self.g.kernel_name() == before, "a refused set_mode keeps the mode"
        if kernel is not None:
            assert self.g.kernel_name() == kernel, "kernel_name %s, expected %s" % (self.g.kernel_name(), kernel)
        return want

    def set_fm(self, deviation, amplitude, tone_level, tone_steps):
        assert self.g.set_fm(deviation, amplitude, tone_level, tone_steps) == 0
        self._both(True, "set_fm", deviation, amplitude, tone_level, tone_steps)
        self.fm_set = True

    def set_cw(self, **kw):
        assert self.g.set_cw(**kw) == 0
        self._both(True, "set_cw", **kw)
        self.cw_set = True

    def set_in(self, **kw):
        assert self.g.set_in(**kw) == 0
        self._both(False, "set_in", **kw)
        self.in_set = True

    def clear_in(self):
        assert self.g.clear_in() == 0
        self._both(False, "clear_in")
        self.in_set = False

    def reset(self):
        assert self.g.reset() == 0
        self._both(False, "reset")
        self.assert_state("behind reset()")

    def set_phase(self, phase):
        """selenite_tx_set_state with every channel's nco_phase at `phase` (the other arrays as they are)"""
        st = self.g.state()
        st["nco_phase"][:] = phase
        self.g.set_state(st)
        self._both(True, "set_phase", phase)

    # ---- state: the chain's four arrays, then fm.*, cw.* and in.* where they are configured ----
    def gpu_state(self):
        st = self.g.state()
        if self.fm_set:
            st["fm.tone_phase"] = self.g.fm_state()["tone_phase"]
        if self.cw_set:
            st.update({"cw." + k: v for k, v in self.g.cw_state().items()})
        if self.in_set:
            st.update({"in." + k: v for k, v in self.g.in_state().items()})
        return st

    def oracle_state(self):
        so = self.o.chain.state()
        st = {k: so[k] for k in STATE_KEYS}
        if self.fm_set:
            st["fm.tone_phase"] = so["tone_phase"]
        else:
            assert not so["tone_phase"].any()
        if self.cw_set:
            st.update({"cw." + k: so[k] for k in ("key_state", "side_phase", "tx_on", "hold")})
        if self.in_set:
            st.update({"in." + k: v for k, v in self.o.in_state().items()})
        return st

    def restore(self, st):
        self.g.set_state({k: st[k] for k in STATE_KEYS})
        if self.fm_set:
            self.g.set_fm_state({"tone_phase": st["fm.tone_phase"]})
        if self.cw_set:
            self.g.set_cw_state({k[3:]: v for k, v in st.items() if k.startswith("cw.")})
        if self.in_set:
            self.g.set_in_state({k[3:]: v for k, v in st.items() if k.startswith("in.")})

    def assert_state(self, what=""):
        sg, so = self.gpu_state(), self.oracle_state()
        assert set(sg) == set(so), (sorted(sg), sorted(so))
        for k in so:
            assert_bits(sg[k], np.asarray(so[k], sg[k].dtype) if k == "cw.key_state" else so[k], "state %s %s" % (k, what))

    def _done(self):
        assert self.g.sync() == 0, "sync()"
        self.g.check()

    def _on_split16(self, served):
        on = self.split and served == "split16"
        assert not on or self.matrix
        return on

    # ---- the audio entries ----
    def gpu_audio(self, x, device=False):
        g, q15 = self.g, x.dtype == np.int16
        if not device:
            y = g.process_q15(x) if q15 else g.process(x)
        else:
            nch, bs = x.shape
            shape = (nch, bs * self.spec.interp, 2)
            d_in, d_out = self.sr.DeviceBuffer(x.nbytes), self.sr.DeviceBuffer(int(np.prod(shape)) * x.itemsize)
            d_in.upload(x)
            (g.L.selenite_tx_process_q15_device if q15 else g.L.selenite_tx_process_f32_device)(g.h, d_in.ptr, d_out.ptr, bs)
            assert g.sync() == 0
            y = d_out.download(shape, x.dtype)
            d_in.free()
            d_out.free()
        self._done()
        return (y,)

    def call(self, x, device=False, served=None, what="", gpu=None):
        """served: the kernel family that must serve the call, where the caller knows it (ez.walk); None: from the host's rule.
        gpu: what the GPU gave for this call, where the caller has made it already (checkpoint)"""
        q15 = x.dtype == np.int16
        if served is None:
            served = self.served_by_rule(x.shape[1])
        (y,) = self.gpu_audio(x, device) if gpu is None else gpu
        want, ref = [(o.chain.process_q15(x) if q15 else o.chain.process(x)) if o is not None else None for o in (self.o, self.oc)]
        self._rephase()
        assert_iq(y, want, ref, self._on_split16(served), q15, served, what)
        self.assert_state(what)
        return (y,)

    def served_by_rule(self, bs):
        served = fz.FAMILY[self.g.kernel_name()]
        return "generic" if served in ("fused", "split16") and bs % 256 else served

    # ---- the key entries ----
    def gpu_key(self, keys, side=None, q15=False, device=False):
        """-> (I/Q, the sidetone buffer behind the call or None)"""
        g = self.g
        nch, n = keys.shape
        dt = np.int16 if q15 else np.float32
        if not device:
            rcode, iq, sd = g.process_key_host(keys, side, q15=q15)
            assert rcode == 0, "key call: status %d" % rcode
        else:
            d_k, d_iq = self.sr.DeviceBuffer(keys.nbytes), self.sr.DeviceBuffer(nch * n * self.spec.interp * 2 * np.dtype(dt).itemsize)
            d_k.upload(keys)
            d_s = None
            if side is not None:
                d_s = self.sr.DeviceBuffer(side.nbytes)
                d_s.upload(np.ascontiguousarray(side, dt))
            assert g.process_key(d_k.ptr, d_iq.ptr, d_s.ptr if d_s else None, n, q15=q15) == 0
            assert g.sync() == 0
            iq, sd = d_iq.download((nch, n * self.spec.interp, 2), dt), (d_s.download((nch, n), dt) if d_s else None)
            for b in (d_k, d_iq, d_s):
                if b is not None:
                    b.free()
        self._done()
        return iq, sd

    def key_call(self, keys, side=None, q15=False, device=False, what="", gpu=None):
        """k_tx_cw serves every key call, on a SPLIT16 instance as FMA: I/Q and sidetone on bits in every arithmetic"""
        iq, sd = self.gpu_key(keys, side, q15, device) if gpu is None else gpu
        want_iq, want_sd = self.o.chain.process_key(keys, side, q15)
        if self.oc is not None:
            self.oc.chain.process_key(keys, side, q15)
        self._rephase()
        assert_bits(iq, want_iq, "%s output (cw)" % what)
        assert (side is None and sd is None) or (sd is not None and want_sd is not None)
        if side is not None:
            assert_bits(sd, want_sd, "%s sidetone" % what)
        self.assert_state(what)
        return iq, sd

    # ---- the frame entries ----
    def gpu_frames(self, frames, entry):
        """entry: "f32_dev", "q15_dev", "q15f_dev", "f32_host", "q15_host" -> (the stage's audio, I/Q)"""
        g = self.g
        kind, host = KINDS[entry.split("_")[0]], entry.endswith("_host")
        nch = frames.shape[0]
        bs = frames.shape[1] // (g._in_M * g._in_fw)
        odt = np.int16 if kind == tio.K_Q15 else np.float32
        if host:
            rcode, iq = g.process_frames_host(frames, q15=kind == tio.K_Q15)
            assert rcode == 0, "frame call: status %d" % rcode
        else:
            d_f, d_iq = self.sr.DeviceBuffer(frames.nbytes), self.sr.DeviceBuffer(nch * bs * self.spec.interp * 2 * np.dtype(odt).itemsize)
            d_f.upload(frames)
            assert g.process_frames(d_f.ptr, d_iq.ptr, bs, kind) == 0
            assert g.sync() == 0
            iq = d_iq.download((nch, bs * self.spec.interp, 2), odt)
            d_f.free()
            d_iq.free()
        self._done()
        a = np.empty((nch, bs), odt)
        assert self.sr.lib().selenite_rx_memcpy_d2h(a.ctypes.data, g.in_audio_device(), a.nbytes) == 0
        return a, iq

    def frame_call(self, frames, entry, served=None, what="", gpu=None):
        kind = KINDS[entry.split("_")[0]]
        if served is None:
            served = self.served_by_rule(frames.shape[1] // (self.g._in_M * self.g._in_fw))
        a, iq = self.gpu_frames(frames, entry) if gpu is None else gpu
        want_a, want_iq = self.o.process_frames(frames, kind)
        ref = self.oc.process_frames(frames, kind)[1] if self.oc is not None else None
        self._rephase()
        assert_bits(a, want_a, "%s the stage's audio" % what)
        assert_iq(iq, want_iq, ref, self._on_split16(served), kind == tio.K_Q15, served, what)
        self.assert_state(what)
        return a, iq

    # ---- a checkpoint over any call ----
    def checkpoint(self, gpu_call, full_call, what=""):
        """every state array, the call, restore, the same call again: the bits and the state of the first time.  gpu_call(): the GPU's
        part alone -> arrays; full_call(gpu=...): the comparison against the oracle"""
        snap = self.gpu_state()
        first = full_call(gpu=gpu_call())
        after = self.gpu_state()
        self.restore(snap)
        again = self.gpu_state()
        for k in snap:
            assert_bits(again[k], snap[k], "%s restored %s" % (what, k))
        for got, was in zip(gpu_call(), first):
            if was is not None:
                assert_bits(got, was, what + " replay behind the restore")
        again = self.gpu_state()
        for k in after:
            assert_bits(again[k], after[k], "%s state %s behind the replay" % (what, k))
        return first

    # ---- refusals: the host's own ARGUMENT_ERROR paths, which launch nothing.  The status latches: the instance is done with ----
    def _refused(self, call, nbytes_iq, nbytes_side, what):
        d_iq, d_s = self.sr.DeviceBuffer(nbytes_iq), self.sr.DeviceBuffer(nbytes_side)
        fill_iq, fill_s = np.full(nbytes_iq, 0x5A, np.uint8), np.full(nbytes_side, 0xA5, np.uint8)
        d_iq.upload(fill_iq)
        d_s.upload(fill_s)
        before = self.gpu_state()
        assert call(d_iq.ptr, d_s.ptr) == rc.ARGUMENT_ERROR, what + ": status"
        assert self.g.sync() == rc.ARGUMENT_ERROR, what + ": the refusal is recorded"
        assert_bits(d_iq.download((nbytes_iq,), np.uint8), fill_iq, what + ": the destination")
        assert_bits(d_s.download((nbytes_side,), np.uint8), fill_s, what + ": the sidetone buffer")
        now = self.gpu_state()
        assert set(now) == set(before)
        for k in before:
            assert_bits(now[k], before[k], "%s: state %s" % (what, k))
        self.assert_state(what)
        d_iq.free()
        d_s.free()

    def refused_key(self, q15=False, what=""):
        nch, n, isz = self.spec.channels, self.spec.block, 2 if q15 else 4
        d_k = self.sr.DeviceBuffer(nch * n)
        d_k.upload(np.ones((nch, n), np.uint8))
        self._refused(lambda iq, sd: self.g.process_key(d_k.ptr, iq, sd, n, q15=q15), nch * n * self.spec.interp * 2 * isz, nch * n * isz, what)
        d_k.free()

    def refused_frames(self, entry, what=""):
        """behind clear_in: ARGUMENT_ERROR whatever the frames are"""
        nch, n = self.spec.channels, self.spec.block
        d_f = self.sr.DeviceBuffer(nch * n * 8 * 2 * 4)
        d_f.upload(np.zeros(nch * n * 8 * 2, np.float32))
        self._refused(lambda iq, sd: self.g.process_frames(d_f.ptr, iq, n, KINDS[entry.split("_")[0]]), nch * n * self.spec.interp * 2 * 4, 16, what)
        d_f.free()


def run_entry_case(case):
    """Every event of an ez case on an EntryPair; an assertion carries the whole case and the event index"""
    i, p = -1, None
    try:
        p = EntryPair(ez.build_spec(case), kernel=ez.expected_kernel(case))
        if case["fm"]:
            p.set_fm(*ez.fm_args(case["fm"]))
        if case["cw"]:
            p.set_cw(**ez.cw_args(case["cw"]))
        if case["inp"]:
            p.set_in(**ez.in_args(case["inp"]))
        served, cw, inp = {}, case["cw"], case["inp"]
        for ei, rec in ez.walk(case):
            served[ei] = rec["kernel"]
        for i, ev in enumerate(case["events"]):
            op, what = ev["op"], "event %d (%s)" % (i, ev["op"])
            if op == "set_mode":
                assert p.set_mode(ev["mode"], ez.expected_kernel(case, ev["mode"])) == 0
            elif op == "set_cw":
                cw = ev["cw"]
                p.set_cw(**ez.cw_args(cw))
            elif op == "set_in":
                inp = ev["inp"]
                p.set_in(**ez.in_args(inp))
            elif op == "clear_in":
                p.clear_in()
            elif op == "reset":
                p.reset()
            elif op == "set_phase":
                p.set_phase(ev["phase"])
            elif op == "process":
                p.call(ez.audio(case, ev), ev["device"], served[i], what)
            elif op in ("key", "key_checkpoint"):
                assert served[i] == "cw"
                k, side = ez.keys(case, ev), (ez.side_in(case, ev) if cw["side"] != "none" else None)
                if op == "key":
                    p.key_call(k, side, ev["q15"], ev["device"], what)
                else:
                    p.checkpoint(lambda: p.gpu_key(k, side, ev["q15"], ev["device"]),
                                 lambda gpu: p.key_call(k, side, ev["q15"], ev["device"], what, gpu), what)
            elif op in ("frames", "frames_checkpoint"):
                x = ez.frames(case, ev, inp)
                if op == "frames":
                    p.frame_call(x, ev["entry"], served[i], what)
                else:
                    p.checkpoint(lambda: p.gpu_frames(x, ev["entry"]), lambda gpu: p.frame_call(x, ev["entry"], served[i], what, gpu), what)
            elif op == "refused_key":
                p.refused_key(ev["q15"], what)
            else:
                assert op == "refused_frames", op
                p.refused_frames(ev["entry"], what)
    except AssertionError as e:
        raise AssertionError("%s\n  at event %d of case %r" % (e, i, case)) from e
    finally:
        if p is not None:
            p.close()
