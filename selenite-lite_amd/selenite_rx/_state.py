"""The state round trip every object shares: a *_state_view struct of the C-ABI filled from a dict of numpy arrays, driven by the
struct's own _fields_ (the member's pointer type gives the dtype), and the get / set calls on top of it."""
import ctypes as C

import numpy as np

from . import RxError



def dtypes(view_cls):
    """member -> numpy scalar type, from the pointer types of the view struct"""
    return {name: np.dtype(ptr._type_).type for name, ptr in view_cls._fields_}


def channel_rows(view_cls, channels):
    """member -> (channels,): the shapes of a view whose members hold one value per channel (dict(channel_rows(...), m=...) for the rest)"""
    return {name: (channels,) for name, _ in view_cls._fields_}


def view(view_cls, shapes, arrays):
    """(view, kept): a view_cls whose members point at `arrays`, each made contiguous in its member's dtype and checked against
    shapes[member]; a member that `arrays` lacks (or gives as None) stays NULL, which the library reads as "leave it as it is".  A member
    without elements passes its array's address like any other: the library copies no row of no bytes.  `kept` holds the arrays the
    pointers refer to; keep it until the call has returned."""
    v, kept = view_cls(), {}
    for name, ptr in view_cls._fields_:
        if arrays.get(name) is None:
            continue
        a = np.ascontiguousarray(arrays[name], np.dtype(ptr._type_))
        if a.shape != tuple(shapes[name]):
            raise ValueError("%s: %s expected, not %s" % (name, tuple(shapes[name]), a.shape))
        kept[name] = a
        setattr(v, name, a.ctypes.data_as(ptr))
    return v, kept


def _call(fn, h, v, err):
    rc = fn(h, C.byref(v))
    if rc:
        raise RxError(rc, fn.__name__ if err is None else err() if callable(err) else err)


def get_state(fn, h, view_cls, shapes, err=None):
    """every member of view_cls as a zeroed array of shapes[member], filled by fn(h, view).  A failure raises RxError with the text `err`
    (a callable: what it returns; None: the symbol's name)."""
    v, arrays = view(view_cls, shapes, {name: np.zeros(shapes[name], t) for name, t in dtypes(view_cls).items()})
    _call(fn, h, v, err)
    return arrays


def set_state(fn, h, view_cls, shapes, arrays, err=None):
    """fn(h, view) on the members `arrays` gives; the others are left as they are"""
    v, kept = view(view_cls, shapes, arrays)
    _call(fn, h, v, err)
