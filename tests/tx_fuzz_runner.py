"""One GPU TX instance and its oracle side by side (tests/test_gpu_tx_fuzz.py, tests/test_gpu_tx_edges.py): every operation goes to both,
every call is compared -- output, every state array, the status -- as the arithmetic of the instance allows:

    SELENITE_ARITH_CMSIS / _FMA   output and state on bits against txfm_oracle.TxFmOracle of the same arithmetic
    SELENITE_ARITH_SPLIT16        state on bits against the FMA oracle (tests/test_gpu_tx.py: test_tx_split16_interpolator_on_the_matrix_pipe);
                                  output on bits against the FMA oracle wherever k_tx_split16 does not serve the call (FM, k_tx_generic,
                                  a shape without the matrix kernel); a call on k_tx_split16 against the CMSIS oracle, per channel and per
                                  256 complex outputs max|gpu - ref| <= TOL max|ref| (f32; TOL of tests/test_gpu_tx.py), at most 1 LSB (int16)

The CMSIS oracle of a SPLIT16 instance takes both phase accumulators from the FMA oracle behind every call: in FM the phase is the running
sum of the modulation, the two arithmetics round the modulating signal differently, and a reference that starts a later call from another
phase is no reference for it.  Its filter states stay its own, as in the existing split16 tests.

TEST INFRASTRUCTURE.  Nothing here is imported by the product.
"""
import copy

import numpy as np

import rxcommon as rc
import tx_fuzz_cases as fz
import txfm_oracle as fo
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
