"""The one filler of the request records of include/drgnn.h (the ``_lib.*Request`` classes).

Every entry point that takes a record validates the ``host_<x>`` copy of an index table and then launches a kernel that
indexes through the device copy ``<x>`` unchecked, so the two must hold the same values: ``Request.table`` makes the host
copy once, uploads exactly that copy and sets both fields, and no other line of the package assigns a ``host_*`` field
of a request.  An empty table or tensor is passed as NULL, on both sides.
"""
import numpy as np
import torch

from . import _lib

_NUMPY = {torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32, torch.float64: np.float64,
          torch.uint8: np.uint8}


class Request(object):
    """A fresh record ``q`` of the class ``record`` for calls on ``device``, and ``held``: every array and tensor ``q``
    points into, kept alive as long as the Request or ``q`` itself is."""

    def __init__(self, record, device):
        self.q, self.device, self.held = record(), torch.device(device), []
        self.q._held = self.held

    def _set(self, name, value):
        if not hasattr(type(self.q), name):                            # (ctypes would take a misspelt name silently)
            raise AttributeError("%s has no field %r" % (type(self.q).__name__, name))
        setattr(self.q, name, value)

    def set(self, **scalars):
        """the scalar fields, by name"""
        for name, value in scalars.items():
            self._set(name, value)

    def _point(self, name, t):
        self._set(name, t.data_ptr() if t.numel() else None)
        self.held.append(t)
        return t

    def _host(self, name, array, dtype, shape):
        host = np.ascontiguousarray(array, dtype=_NUMPY[dtype]).reshape(shape)
        self._set("host_" + name, host.ctypes.data if host.size else None)
        self.held.append(host)
        return host

    def table(self, name, array, dtype=torch.int32, shape=(-1,), device_copy=None):
        """A checked table: (host, device) with ``host`` the contiguous copy of ``array`` the library validates
        (``q.host_<name>``) and ``device`` the upload of exactly that copy (``q.<name>``).  ``device_copy``: a tensor on
        the device the caller already holds for the same array."""
        host = self._host(name, array, dtype, shape)
        if device_copy is None:
            device_copy = torch.from_numpy(host).to(self.device)
        elif (device_copy.dtype != dtype or device_copy.numel() != host.size or not device_copy.is_contiguous() or
              device_copy.device.type != self.device.type):
            raise ValueError("the device copy of %s must be %s [%d] on %s" % (name, dtype, host.size, self.device))
        return host, self._point(name, device_copy)

    def host_table(self, name, array, dtype=torch.int32, shape=(-1,)):
        """a table that exists on the host only (``q.host_<name>`` without a ``q.<name>``)"""
        return self._host(name, array, dtype, shape)

    def input(self, name, value, dtype=None, shape=None, error=None):
        """A plain input: an array to upload as ``dtype``, or a tensor already on the device; made contiguous and, with
        ``dtype``, held to it and to ``shape`` (None: any extent) by ValueError(``error``).  None leaves the field NULL."""
        if value is None:
            return None
        if not torch.is_tensor(value):
            value = torch.from_numpy(np.ascontiguousarray(value, dtype=_NUMPY[dtype])).to(self.device)
        value = value.contiguous()
        if dtype is not None and (value.dtype != dtype or (shape is not None and (
                value.dim() != len(shape) or any(s is not None and s != v for s, v in zip(shape, value.shape))))):
            raise ValueError(error)
        return self._point(name, value)

    def output(self, names, shape, dtype, zeros=False):
        """A freshly allocated output (``zeros``: cleared); ``names``: the field, or a tuple of fields that get one row
        each of the leading axis."""
        out = (torch.zeros if zeros else torch.empty)(shape, dtype=dtype, device=self.device)
        if isinstance(names, str):
            return self._point(names, out)
        for name, row in zip(names, out):
            self._point(name, row)
        return out

    def stream(self):
        """the raw hipStream_t of torch's current stream on the device (None on the host)"""
        return torch.cuda.current_stream(self.device).cuda_stream if self.device.type == "cuda" else None

    def run(self, api, method):
        """``api.<method>(q, stream)``; the product library takes tensors of the GPU only"""
        if api is _lib._API:
            _lib.require_device(*[t for t in self.held if torch.is_tensor(t)])
        getattr(api, method)(self.q, self.stream())
