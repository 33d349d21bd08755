"""What the modules of the Python host mirror share: the Python counterpart of csrc/conv3p_host.hpp.

The errors and the status-to-exception call, the device check, one scratch-pool function, the two pointer idioms of the
C ABI (the current stream's handle; a tensor's address or NULL), the argument checks that every entry point repeats -- a
tensor of a dtype, shape and device; an integer in a range -- each given the message of its call site, the growing
scratch buffer an output object keeps, and the view-maker behind the output classes' trim() and room().  conv3p_op.py
re-exports the names it used to define.
"""
import ctypes

import torch

from . import _lib


class Conv3pInvalidArgument(ValueError):
    """Analogue of tf.errors.InvalidArgumentError raised by the op's OP_REQUIRES checks."""


class Conv3pRuntimeError(RuntimeError):
    pass


_SFX = {torch.float32: ("f32", ctypes.c_float, 4), torch.float64: ("f64", ctypes.c_double, 8)}
_LABEL_DTYPES = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}       # label dtype -> its bytes, as the C ABI takes it


def _require(cond, msg):
    if not cond:
        raise Conv3pInvalidArgument(msg)


def _call(fn, *args):
    rc = fn(*args)
    if rc == _lib.OK:
        return
    msg = "conv3p: %s (status %d)" % (_lib.status_string(rc), rc)
    if rc == _lib.ERR_INVALID_ARGUMENT:
        raise Conv3pInvalidArgument(msg)
    raise Conv3pRuntimeError(msg)


def _check_device(*tensors):
    dev = tensors[0].device
    if dev.type != "cuda":
        raise Conv3pRuntimeError("conv3p: tensors must live on a HIP device (no CPU path in pointwise_amd)")
    for t in tensors:
        if t.device != dev:
            raise Conv3pRuntimeError("conv3p: all tensors must be on the same device")
    return dev


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _ptr(t, when=True):
    """The tensor's address for the C ABI, NULL (None) for a missing or empty tensor or when `when` is false."""
    return t.data_ptr() if when and t is not None and t.numel() else None


def _upload(host, dev):
    """A small CPU tensor a call was given as host data -> its copy on `dev`, enqueued on the current stream without the
    host waiting for the device (the stream contract): the values are staged in pinned memory and
    copied from there asynchronously; torch's pinned allocator keeps the staging block until the copy's event has passed.
    A pageable .to(dev) would be followed by a stream synchronise."""
    return host.pin_memory().to(dev, non_blocking=True)


def _workspace(dev, nbytes, pool):
    """The caller-owned workspace of the C ABI: pool's growing scratch buffer for (device, current stream).  A pool is a
    dict its module owns; the conv3p op and the heads keep separate ones."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    buf = pool.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = pool[key] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
    return buf


_HEADS = {}   # the pool head.py, seg_head.py and optim.py share; conv3p_op.py keeps its own


def _grow(obj, name, need, dev):
    """obj.<name>, the uint8 scratch tensor an object keeps between calls, made or regrown to `need` bytes -> it."""
    buf = getattr(obj, name, None)
    if buf is None or buf.numel() < need:
        buf = torch.empty(need, dtype=torch.uint8, device=dev)
        setattr(obj, name, buf)
    return buf


def _fill_empty(out):
    """Nothing is launched, so nothing is written: the host gives the tensors of out._FILL, pairs of a name and the value
    the class's docstring states for the entries past the emitted ones, that value."""
    for name, value in out._FILL:
        t = getattr(out, name)
        if t is not None:
            t.fill_(value) if value else t.zero_()


def _is_tensor(t, dtype, shape=None, dev=None, ndim=None, min_dim=None, contiguous=True):
    """A tensor of `dtype` (one, or a container of several), and, where given: of exactly `shape`, of `ndim` / at least
    `min_dim` dimensions, on `dev`, contiguous."""
    return (isinstance(t, torch.Tensor) and (t.dtype == dtype if isinstance(dtype, torch.dtype) else t.dtype in dtype)
            and (shape is None or tuple(t.shape) == tuple(shape)) and (ndim is None or t.dim() == ndim)
            and (min_dim is None or t.dim() >= min_dim) and (dev is None or t.device == dev)
            and (not contiguous or t.is_contiguous()))


def _require_tensor(t, msg, dtype, shape=None, dev=None, **kw):
    _require(_is_tensor(t, dtype, shape, dev, **kw), msg)


def _is_int(v, lo, hi, allow_bool=False):
    """An int in [lo, hi]; a bool is one only where the call has always taken it."""
    return isinstance(v, int) and (allow_bool or not isinstance(v, bool)) and lo <= v <= hi


def _require_int(v, msg, lo, hi, allow_bool=False):
    _require(_is_int(v, lo, hi, allow_bool), msg)


def _view(obj, cls, rows, sliced, shared, **fixed):
    """A `cls` made without its constructor, as trim() and room() hand out: the `sliced` attributes are obj's cut to the
    slice `rows` along the first axis (None stays None; one obj does not have, as _neigh before its first use, is not
    set), the `shared` ones are obj's own objects, and `fixed` are set as given."""
    t = object.__new__(cls)
    for name in sliced:
        if hasattr(obj, name):
            v = getattr(obj, name)
            setattr(t, name, v[rows] if v is not None else None)
    for name in shared:
        setattr(t, name, getattr(obj, name))
    vars(t).update(fixed)
    return t
