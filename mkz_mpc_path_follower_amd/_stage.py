"""Host plumbing the loop stages share (vehicle_sim, ref_traj, closed_loop): what a kernel may be handed as a raw pointer, how it is handed over,
and how a table of per-vehicle rows is built from the library's default row.  Private: the stages' public names, texts and defaults stay where
they are -- a call site keeps its own refusal text and its own order of checks, and only asks here whether a tensor is what it must be.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


def device_of(device):
    """an index -> that MI355X; anything else as torch.device takes it"""
    return torch.device("cuda", device) if isinstance(device, int) else torch.device(device)


def is_buffer(t, dtype, shape, device):
    """the tensor contract of every stage: `t` is a torch tensor of `dtype` (one dtype, or a tuple of admissible ones) with exactly `shape`,
    contiguous, on `device` -- what reaches a kernel is its raw pointer, so nothing less will do.  A subclass of torch.Tensor is a tensor.
    A control period asks this some sixty times, so the usual case (one dtype, and it matches) is tried first and the shape is compared as it is."""
    return (isinstance(t, torch.Tensor) and (t.dtype == dtype or (type(dtype) is tuple and t.dtype in dtype)) and t.shape == shape
            and t.is_contiguous() and t.device == device)


def ptr(t):
    """the tensor's address as the library takes it; None stays None (an optional buffer not given)"""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream(device):
    """torch's current stream on `device`, as the library takes it: every stage launches there"""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def default_row(entry, words):
    """one default row [words] from the library's `entry` (kmpc_*_default), whichever of the two calling conventions it has: (row) or (rows, n).
    The row starts as NaN, so a word the library did not write would not pass for a default."""
    row = np.full(words, np.nan)
    fn = getattr(_lib.load(), entry)
    _lib.check(fn(row.ctypes.data_as(C.POINTER(C.c_double)), *((1,) if len(fn.argtypes) == 2 else ())))
    return row


def host_rows(rows):
    """a tensor on any device, or anything numpy takes for an array -> float64 numpy rows on the host (what the check_* functions validate)"""
    return np.asarray(rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else rows, dtype=np.float64)


def rows_of(bad):
    """a mask over the rows -> the first eight offending row indices, as the check_* functions list them"""
    return np.flatnonzero(bad)[:8].tolist()


def table_rows(name, fields, default, B, overrides, groups=None, conflict=None):
    """A row table: the `default` row tiled B times, with each override a scalar or one value per vehicle -> [B,words] host rows, not yet validated
    (the table's own check_* does that).  `fields` names the words in row order.  `groups` maps a key that sets several words at once to their
    indices (road's `mu`, the fault row's `p_lose` ...); giving a group together with one of its members is refused with `conflict` % the key.
    `name` is the caller's, for the texts."""
    groups = groups or {}
    rows = np.tile(default, (int(B), 1))
    for k, v in overrides.items():
        if k not in groups and k not in fields:
            raise ValueError("%s: unknown parameter %r (%sone of %s)" % (name, k, ", ".join(groups) + " or " if groups else "", ", ".join(fields)))
        words = groups[k] if k in groups else (fields.index(k),)
        if k in groups and any(fields[w] in overrides for w in words):
            raise ValueError("%s: %s" % (name, conflict % k))
        v = np.asarray(v, dtype=np.float64)
        if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != int(B)):
            raise ValueError("%s: %s is a scalar or one value per vehicle [%d], got %s" % (name, k, B, v.shape))
        for w in words:
            rows[:, w] = v
    return rows


def fill_blocks(name, rows, blocks, values=None):
    """each block (key, v, c0, w) of a stage's constructor -- v a scalar, w values or [B,w] -- into the columns c0 ... c0 + w - 1 of `rows` [B,W], in
    place.  `values` words "w values" in the refusal where a stage says more (the sensor's and the estimator's "four values (x, y, psi, v)")."""
    B = rows.shape[0]
    for key, v, c0, w in blocks:
        v = np.asarray(v, dtype=np.float64)
        if v.shape not in ((), (w,), (B, w)):
            raise ValueError("%s: %s is a scalar, %s or [%d,%d], got %s" % (name, key, values or "%d values" % w, B, w, v.shape))
        rows[:, c0:c0 + w] = v
    return rows
