"""CPU: the pieces the objects of the ctypes binding share -- the state-view helper (selenite_rx._state), the dtype tables derived from the
view structs, the signature table lib() binds from (selenite_rx.SIGNATURES) -- and what importing the package must not do.  No
instance, no GPU."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import rxcommon as rc
import selenite_rx as sr
from selenite_rx._state import dtypes, view

ABI_LISTS = sorted(k for k in dir(sr) if k.endswith("ABI_SYMBOLS"))


def addr(p):
    return C.cast(p, C.c_void_p).value


NB_SHAPES = dict(level=(3,), blanked=(3,), bursts=(3,))
CWDEC_SHAPES = dict({k: (3,) for k in ("peak", "floor", "primed", "key", "flip", "run", "unit", "code", "word", "count")}, text=(3, 8))


def zeros(view_cls, shapes):
    return {k: np.zeros(shapes[k], t) for k, t in dtypes(view_cls).items()}


@pytest.mark.parametrize("view_cls,shapes", [(sr.NbStateView, NB_SHAPES), (sr.CwdecStateView, CWDEC_SHAPES)], ids=["nb", "cwdec"])
def test_view_points_at_the_arrays_it_is_given(view_cls, shapes):
    a = zeros(view_cls, shapes)
    v, kept = view(view_cls, shapes, a)
    assert list(kept) == [n for n, _ in view_cls._fields_]
    for name, ptr in view_cls._fields_:
        assert kept[name] is a[name]                                        # right dtype, contiguous: no copy
        assert isinstance(getattr(v, name), ptr) and addr(getattr(v, name)) == a[name].ctypes.data, name


@pytest.mark.parametrize("view_cls,shapes", [(sr.NbStateView, NB_SHAPES), (sr.CwdecStateView, CWDEC_SHAPES)], ids=["nb", "cwdec"])
def test_view_leaves_an_absent_member_null(view_cls, shapes):
    names = [n for n, _ in view_cls._fields_]
    for given in names:
        a = zeros(view_cls, shapes)
        v, kept = view(view_cls, shapes, {given: a[given], names[0 if given != names[0] else 1]: None})     # (None counts as absent)
        assert list(kept) == [given]
        for n in names:
            assert (addr(getattr(v, n)) == a[given].ctypes.data) if n == given else (addr(getattr(v, n)) is None), (given, n)
    v, kept = view(view_cls, shapes, {})
    assert not kept and all(addr(getattr(v, n)) is None for n in names)


def test_view_refuses_a_wrong_shape():
    for bad in (np.zeros(4, np.float32), np.zeros((3, 1), np.float32), np.zeros((), np.float32)):
        with pytest.raises(ValueError):
            view(sr.NbStateView, NB_SHAPES, {"level": bad})
    for bad in (np.zeros((3, 7), np.uint8), np.zeros((8, 3), np.uint8), np.zeros(24, np.uint8)):
        with pytest.raises(ValueError):
            view(sr.CwdecStateView, CWDEC_SHAPES, {"text": bad})
    with pytest.raises(ValueError):
        view(sr.CwdecStateView, CWDEC_SHAPES, {"count": np.zeros(2, np.uint64)})


def test_view_converts_what_it_cannot_point_at():
    """a wrong dtype or a non-contiguous array is copied into the member's dtype, contiguous; the pointer is the copy's"""
    wide = np.arange(6, dtype=np.float64)
    strided = np.arange(6, dtype=np.uint64)[::2]
    v, kept = view(sr.NbStateView, NB_SHAPES, {"level": wide[:3], "blanked": strided, "bursts": [7, 8, 9]})
    for name, src, dt in (("level", wide[:3], np.float32), ("blanked", strided, np.uint64), ("bursts", np.array([7, 8, 9]), np.uint64)):
        k = kept[name]
        assert k.dtype == dt and k.flags.c_contiguous and k.shape == (3,) and np.array_equal(k, src)
        assert not np.shares_memory(k, src) and addr(getattr(v, name)) == k.ctypes.data
    text = np.arange(48, dtype=np.uint8).reshape(3, 16)[:, ::2]                 # right dtype and shape, wrong strides
    units = np.array([1.0, 2.0, 3.0], np.float32)                               # whole numbers in the wrong dtype
    v, kept = view(sr.CwdecStateView, CWDEC_SHAPES, {"text": text, "unit": units})
    assert kept["text"].flags.c_contiguous and np.array_equal(kept["text"], text) and not np.shares_memory(kept["text"], text)
    assert kept["unit"].dtype == np.uint32 and kept["unit"].tolist() == [1, 2, 3]
    assert addr(v.text) == kept["text"].ctypes.data and addr(v.unit) == kept["unit"].ctypes.data and addr(v.peak) is None


def test_dtype_tables_are_what_was_written_by_hand():
    """Rx.*_TYPES come from the view structs now; these are the dicts the class spelled out before, in their order"""
    meter = dict(level=np.float32, open=np.uint32, hold=np.uint32, opens=np.uint64, open_blocks=np.uint64)
    tones = dict(s=np.float32, energy=np.float32, power=np.float32, frame_energy=np.float32, last_best=np.uint32, tone=np.uint32,
                 cand=np.uint32, run=np.uint32, changes=np.uint64, position=np.uint64)
    cwdec = dict(peak=np.float32, floor=np.float32, primed=np.uint32, key=np.uint32, flip=np.uint32, run=np.uint32, unit=np.uint32,
                 code=np.uint32, word=np.uint32, count=np.uint64, text=np.uint8)
    for got, want in ((sr.Rx.METER_TYPES, meter), (sr.Rx.TONES_TYPES, tones), (sr.Rx.CWDEC_TYPES, cwdec)):
        assert got == want and list(got) == list(want)
        assert all(got[k] is want[k] for k in want)
    assert dtypes(sr.RingStateView) == dict(i=np.int16, q=np.int16, buff_enable=np.uint8, rd_ptr=np.uint16, wr_ptr=np.uint16)


def test_pointer_types_are_defined_once():
    for name, t in (("f32p", C.c_float), ("u32p", C.c_uint32), ("i16p", C.c_int16), ("u64p", C.c_uint64), ("u8p", C.c_uint8)):
        assert getattr(sr, name) is C.POINTER(t)


def test_every_declared_symbol_has_a_signature():
    assert len(ABI_LISTS) == 9
    declared = [n for k in ABI_LISTS for n in getattr(sr, k)]
    assert len(set(declared)) == len(declared)
    assert set(declared) == set(sr.SIGNATURES)
    for name, (restype, argtypes) in sr.SIGNATURES.items():
        assert isinstance(argtypes, list) and all(isinstance(a, type) and hasattr(a, "from_param") for a in argtypes), name
        assert restype is None or restype in (C.c_int, C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint64), name
    # a pointer or a string that came back as an int would be cut to 32 bits without a word
    for name in ("selenite_rx_device_alloc", "selenite_rx_host_alloc", "selenite_rx_spectrum_device", "selenite_rx_meter_level_device",
                 "selenite_rx_cwdec_text_device", "selenite_tx_cw_txon_device", "selenite_tx_in_audio_device", "selenite_tx_keyer_key_device"):
        assert sr.SIGNATURES[name][0] is C.c_void_p, name
    for name in declared:
        if name.endswith(("_error_string", "_kernel_name", "_nco_path")):
            assert sr.SIGNATURES[name][0] is C.c_char_p, name
    assert sr.SIGNATURES["selenite_rx_algorithmic_bytes"][0] is C.c_uint64


def test_lib_binds_every_exported_symbol_without_an_instance():
    """the TX and ring prototypes used to be bound by the first Tx(...) / Ring(...); the NULL-instance tests called them before that"""
    L = sr.lib()
    for name, (restype, argtypes) in sr.SIGNATURES.items():
        if hasattr(L, name):
            f = getattr(L, name)
            assert f.argtypes is not None and list(f.argtypes) == argtypes and f.restype is restype, name
    assert all(hasattr(L, n) for n in sr.SIGNATURES)                            # the in-tree library exports all of them
    assert L.selenite_tx_status(None) == sr.ARGUMENT_ERROR and L.selenite_ring_status(None) == sr.ARGUMENT_ERROR
    assert L.selenite_tx_keyer_unit(20.0, 12000.0) == 720 and L.selenite_rx_abi_version() == sr.ABI_VERSION


def test_importing_the_package_opens_nothing():
    code = ("import sys; sys.path.insert(0, %r); import selenite_rx as sr; "
            "assert sr._lib is None and 'torch' not in sys.modules; assert sr.rx.lib is sr.lib and sr.Rx is sr.rx.Rx; print('ok')" % rc.PKG_DIR)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
