"""What the binding checks of a tensor or a row range before the library sees it: the C ABI takes raw device pointers and
cannot tell a device pointer from a host one, so every tensor a caller hands in goes through one of these.  Every refusal
is a ValueError raised before the library is called.  Needs neither the shared library nor a GPU.
"""
import ctypes as C

import torch


def ptr(t):
    """the pointer of a tensor that flat / matrix / vectors has checked, or that the binding allocated itself"""
    return C.c_void_p(t.data_ptr())


def _in_class(t, dtype):
    """beside one torch dtype, `dtype` may be a tuple of them, or 4 / 8 = any integer of that many bytes (asked only when
    t.dtype != dtype, so the usual case costs no call)"""
    if isinstance(dtype, tuple):
        return t.dtype in dtype
    return isinstance(dtype, int) and t.element_size() == dtype and not t.is_floating_point()


def _bad(name, dtype, device, what):
    kind = "%d-byte integer" % dtype if isinstance(dtype, int) else \
        " / ".join(str(d) for d in dtype) if isinstance(dtype, tuple) else str(dtype)
    return ValueError("%s must be a %s tensor on %s %s" % (name, kind, device, what))


def flat(t, dtype, count, device, name, optional=False):
    """pointer of a contiguous tensor of `dtype` on `device` with at least `count` elements (None for None if optional)"""
    if t is None and optional:
        return None
    if not isinstance(t, torch.Tensor) or (t.dtype != dtype and not _in_class(t, dtype)) or not t.is_contiguous() \
            or t.numel() < count or t.device != device:
        raise _bad(name, dtype, device, "that is contiguous and has at least %d entries" % count)
    return C.c_void_p(t.data_ptr())


def matrix(t, dtype, rows, cols, device, name):
    """(pointer, row stride) of a row-major matrix of `dtype` on `device`: at least [rows, cols], last stride 1, row
    stride >= cols (padded rows pass); a contiguous 1-D tensor of rows * cols elements is taken as [rows, cols]"""
    if isinstance(t, torch.Tensor) and (t.dtype == dtype or _in_class(t, dtype)) and t.device == device:
        shape, stride = t.shape, t.stride()              # (each asked once: a call into torch apiece)
        if len(shape) == 2 and shape[0] >= rows and shape[1] >= cols and (cols <= 1 or stride[1] == 1) \
                and stride[0] >= cols:
            return C.c_void_p(t.data_ptr()), stride[0]
        if len(shape) == 1 and shape[0] >= rows * cols and t.is_contiguous():
            return C.c_void_p(t.data_ptr()), cols
    raise _bad(name, dtype, device, "of at least [%d, %d] with contiguous rows" % (rows, cols))


def vectors(t, device, name, m=None):
    """(tensor, count, ld) of int32 vectors on `device` given as [m] or [count, m] with contiguous rows (any row stride
    >= m).  m None: whatever the tensor's last dimension is, with neither it nor count 0."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != device:
        raise ValueError("%s must be an int32 tensor on %s" % (name, device))
    if t.dim() not in (1, 2):
        raise ValueError("%s must be [m] or [count, m]" % name)
    width, count = int(t.shape[-1]), 1 if t.dim() == 1 else int(t.shape[0])
    if m is None and (count == 0 or width == 0):
        raise ValueError("%s must be [m] or [count, m], neither 0" % name)
    if m is not None and width != m:
        raise ValueError("%s must hold m = %d labels a vector" % (name, m))
    ld = int(t.stride(0)) if t.dim() == 2 and count > 1 else width
    if (width > 1 and t.stride(-1) != 1) or ld < width:
        raise ValueError("%s must have contiguous rows (row stride >= m)" % name)
    return t, count, ld


def rows(view_rows, row0, nrows):
    """(row0, n) of the rows [row0, row0 + nrows) of a view of view_rows rows, nrows None = to the view's end.  A negative
    row0 or count is refused (ctypes would wrap it to uint64); a range past the view's end is left to the library."""
    row0 = int(row0)
    n = view_rows - row0 if nrows is None else int(nrows)
    if row0 < 0 or n < 0:
        raise ValueError("rows [%d, %d) outside the view (%d rows)" % (row0, row0 + n, view_rows))
    return row0, n


def index(i, count, name):
    """i as an index into `count` items (a negative one is refused: ctypes would wrap it to uint32)"""
    i = int(i)
    if not 0 <= i < count:
        raise ValueError("%s %d out of range (%d)" % (name, i, count))
    return i
