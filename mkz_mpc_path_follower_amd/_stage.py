"""Host plumbing the loop stages share (vehicle_sim, ref_traj, closed_loop): what a kernel may be handed as a raw pointer, how it is handed over,
how a table of per-vehicle rows is built from the library's default row, and how a record comes back as named fields.  Private: the stages'
public names, texts and defaults stay where they are -- a call site keeps its own refusal text and its own order of checks, and only asks here
whether a tensor is what it must be.  The few refusals worded here (v_cap, out, path_id, present) are those every stage words alike.
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


def is_state_view(t, c, device, rows=None):
    """may the tensor `t` go to a kernel as (pointer, row stride) for its first `c` columns?  float64 on `device`, 2-D with at least c columns (and
    exactly `rows` rows, where given), unit column stride and rows at least c apart: the plant's state [B,8], a column slice of it, an estimate
    [B,4] or a pose [B,3] all pass as they are -- no copy."""
    return (t.dtype == torch.float64 and t.device == device and t.dim() == 2 and t.shape[1] >= c and (rows is None or t.shape[0] == rows)
            and (t.shape[0] == 0 or t.stride(1) == 1) and t.stride(0) >= c)


def state_view(x, c, device, rows, text):
    """`x` as a kernel reads a state: `x` itself where is_state_view says so (the plant's state every period: no copy, no new tensor), else a
    contiguous float64 copy on `device`.  What is then not [rows,W] with W >= c (rows None: any number) is refused with the site's `text`, a format
    for (rows, shape) -- for (shape,) without rows."""
    if type(x) is torch.Tensor and is_state_view(x, c, device, rows):   # every period's case: one question, nothing made
        return x
    st = torch.as_tensor(x, dtype=torch.float64, device=device)
    if not is_state_view(st, c, device):
        st = st.contiguous()
    if st.dim() != 2 or st.shape[1] < c or (rows is not None and st.shape[0] != rows):
        raise ValueError(text % ((tuple(st.shape),) if rows is None else (rows, tuple(st.shape))))
    return st


def cap_in(v_cap, B, device):
    """a stage's speed cap: anything torch takes for a float64 [B] -> a contiguous tensor on `device`"""
    if is_buffer(v_cap, torch.float64, (B,), device):   # every period's case in the loops: their v_target, or a stage's own output
        return v_cap
    vc = torch.as_tensor(v_cap, dtype=torch.float64, device=device).contiguous()
    if tuple(vc.shape) != (B,):
        raise ValueError("v_cap: expected [%d], got %s" % (B, tuple(vc.shape)))
    return vc


def cap_out(out, B, device):
    """a stage's capped speed: the caller's `out` (which must be a buffer) or a new tensor [B]"""
    if out is None:
        return torch.empty((B,), dtype=torch.float64, device=device)
    if not is_buffer(out, torch.float64, (B,), device):
        raise ValueError("out: expected a contiguous float64 tensor [%d] on %s" % (B, device))
    return out


def own_path_id(pid, B, device):
    """a fleet helper's path_id, a plain public attribute: what reaches the kernel is a raw pointer, so it must still be what the helper made"""
    if not is_buffer(pid, torch.int32, (B,), device):
        raise ValueError("path_id must stay a contiguous int32 tensor [%d] on %s (write into it in place)" % (B, device))
    return pid


def check_present(present, B, device):
    """present= of the stages that search the fleet: None (everybody on the road) or one byte per vehicle"""
    if present is not None and not is_buffer(present, (torch.uint8, torch.bool), (B,), device):
        raise ValueError("present: expected a contiguous uint8 or bool tensor [%d] on %s" % (B, device))


def fresh_record(entry, B, words, device):
    """[B,words] float64 on `device` (an index, a name or a torch.device): B fresh records from the library's `entry` (kmpc_*_init)"""
    rec = np.empty((int(B), words))
    _lib.check(getattr(_lib.load(), entry)(rec.ctypes.data_as(C.POINTER(C.c_double)), int(B)))
    return torch.from_numpy(rec).to(device_of(device))


def record_fields(rec, fields, ints=()):
    """a record tensor [B,W] -> its words as named numpy fields [B] (one synchronising download): `fields` names the words in order, `ints` those
    that are counts or indices and come as int64"""
    a = rec.detach().cpu().numpy()
    return {k: a[:, i].astype(np.int64) if k in ints else a[:, i].copy() for i, k in enumerate(fields)}


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
