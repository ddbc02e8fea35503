"""Exact order statistics and quantiles on the device (gpemu_select).

``order_statistics`` returns elements of the input, equal as doubles to ``np.sort(values, axis)[ranks]``;
``quantile`` is ``np.quantile(values, probabilities, axis, method='linear')``: the virtual index and the weight are
computed on the host, the device selects the bracketing order statistics, and the interpolation is numpy's ``_lerp``
expression -- so the two agree up to the rounding of that one expression (exactly where the virtual index is an integer).
numpy arrays go through the host entry; torch tensors that live on the device are read in place through the strided
``_dev`` entry and give a tensor on the same device.  There is no CPU implementation."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr


def check_ranks(ranks, S):
    """``ranks`` as a contiguous int64 vector; ValueError unless every rank is an integer in [0, S)."""
    r = np.asarray(ranks)
    if r.ndim != 1 or r.size == 0:
        raise ValueError("ranks must be a non-empty 1-d sequence")
    if not np.issubdtype(r.dtype, np.integer):
        if not np.all(np.isfinite(r)) or not np.all(r == np.round(r)):
            raise ValueError("ranks must be integers")
    r = np.ascontiguousarray(r, dtype=np.int64)
    if S < 1:
        raise ValueError("order statistics of an empty axis")
    if r.min() < 0 or r.max() >= S:
        raise ValueError(f"every rank must be in [0, {S})")
    return r


def virtual_index(S, probabilities):
    """numpy's ``linear`` virtual index of every probability for ``S`` samples: ``(lo, hi, t)`` with ``lo = floor((S -
    1) p)``, ``hi = min(lo + 1, S - 1)`` and the weight ``t`` in [0, 1) (np.lib._function_base_impl: _compute_virtual_index,
    _get_gamma, _get_indexes)."""
    p = np.asarray(probabilities, dtype=np.float64).reshape(-1)
    if p.size == 0:
        raise ValueError("probabilities must not be empty")
    if not np.all((p >= 0.0) & (p <= 1.0)):     # NaN included
        raise ValueError("Quantiles must be in the range [0, 1]")
    if S < 1:
        raise ValueError("quantiles of an empty axis")
    v = (S - 1) * p
    lo = np.floor(v).astype(np.int64)
    hi = np.minimum(lo + 1, S - 1)
    t = v - lo
    return lo, hi, t


def lerp(a, b, t):
    """numpy's ``_lerp``: ``a + (b - a) t``, or ``b - (b - a) (1 - t)`` where ``t >= 0.5``.  Where the weight is 0 the
    result is ``a`` itself: an integer virtual index returns the element (also next to an infinity, where
    ``(b - a) * 0`` is NaN)."""
    a, b, t = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(t))
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        out = np.where(t >= 0.5, b - d * (1 - t), a + d * t)
    return np.where(t == 0, a, out)


def _bracket(S, probabilities):
    """The distinct ranks the probabilities need and, per probability, where its two ranks are among them."""
    lo, hi, t = virtual_index(S, probabilities)
    ranks, inv = np.unique(np.concatenate([lo, hi]), return_inverse=True)
    return ranks, inv[:lo.size], inv[lo.size:], t


def _flat_rows(values, axis):
    """A float64 device tensor with ``axis`` last and the other axes flattened to rows, for the strided ``_dev`` calls:
    ``(flat (R, S), row stride, element stride, the other axes' shape)`` -- a view where torch can express the rows
    by one stride, else a copy on the device."""
    v = values.movedim(axis, -1)
    S = v.shape[-1]
    lead = v.shape[:-1]
    R = int(np.prod(lead)) if lead else 1
    if R == 0 or S == 0:
        return None, 0, 0, lead
    flat = v.reshape(R, S)
    rs = flat.stride(0) if R > 1 else 1
    es = flat.stride(1) if S > 1 else 1
    if rs <= 0 or es <= 0:      # expanded (stride 0) tensors
        flat = flat.contiguous()
        rs, es = S, 1
    return flat, int(rs), int(es), lead


def _select_tensor(values, ranks, axis):
    """Order statistics of a device tensor along ``axis``, read in place: (n_ranks, *other axes) on the device."""
    import torch
    if values.dtype != torch.float64:
        raise TypeError("device selection needs float64 tensors")
    ranks = check_ranks(ranks, values.shape[axis])
    flat, rs, es, lead = _flat_rows(values, axis)
    if flat is None:
        raise ValueError("no rows to select from")
    R, S = flat.shape
    out = torch.empty((R, ranks.size), dtype=torch.float64, device=values.device)
    check(_lib.lib().gpemu_select_dev(int(values.device.index or 0), R, S, C.c_void_p(flat.data_ptr()), rs, es,
                                      int(ranks.size), ptr(ranks), C.c_void_p(out.data_ptr()),
                                      _lib.current_stream(values.device)))
    return out.reshape(*lead, ranks.size).movedim(-1, 0)


def order_statistics(values, ranks, axis=-1, device=None):
    """The ``ranks``-th smallest elements (0-based) along ``axis``: shape ``(len(ranks), *values.shape without axis)``,
    equal as doubles to ``np.take(np.sort(values, axis), ranks, axis)`` moved to the front.  A slice that holds a NaN
    gives NaN for every rank."""
    if _lib.is_device_tensor(values):
        return _select_tensor(values, ranks, axis)
    _lib.require_device()
    v = np.moveaxis(np.asarray(values, dtype=np.float64), axis, -1)
    S = v.shape[-1] if v.ndim else 0
    if v.ndim == 0:
        raise ValueError("values must have at least one axis")
    ranks = check_ranks(ranks, S)
    lead = v.shape[:-1]
    v = np.ascontiguousarray(v).reshape(-1, S)
    if v.shape[0] == 0:
        raise ValueError("no rows to select from")
    out = np.empty((v.shape[0], ranks.size))
    check(_lib.lib().gpemu_select(int(_lib.resolve_device(device)), v.shape[0], S, ptr(v), int(ranks.size), ptr(ranks),
                                  ptr(out)))
    return np.moveaxis(out.reshape(*lead, ranks.size), -1, 0)


def quantile(values, probabilities, axis=-1, device=None):
    """``np.quantile(values, probabilities, axis=axis, method='linear')`` with the order statistics selected on the
    device: shape ``(len(probabilities), *values.shape without axis)`` (a scalar probability drops the first axis).
    Device tensors give a device tensor (the interpolation of the few selected values runs in torch)."""
    scalar = np.ndim(probabilities) == 0
    S = values.shape[axis]
    ranks, ilo, ihi, t = _bracket(S, probabilities)
    sel = order_statistics(values, ranks, axis=axis, device=device)
    if _lib.is_device_tensor(values):
        import torch
        a, b = sel[torch.as_tensor(ilo, device=sel.device)], sel[torch.as_tensor(ihi, device=sel.device)]
        tt = torch.as_tensor(t, device=sel.device).reshape((-1,) + (1,) * (sel.dim() - 1))
        d = b - a
        out = torch.where(tt >= 0.5, b - d * (1 - tt), a + d * tt)
        out = torch.where(tt == 0, a, out)
        return out[0] if scalar else out
    out = lerp(sel[ilo], sel[ihi], t.reshape((-1,) + (1,) * (sel.ndim - 1)))
    return out[0] if scalar else out


def rankdata(values, axis=-1, device=None, workspace_bytes=0):
    """``scipy.stats.rankdata(values, method='average', axis=axis)``: the average 1-based rank of every element among
    those of its slice along ``axis``, exact (gpemu_rank: a key-only radix sort on the device, then the lower and upper
    bound of every element).  -0 and +0 are tied; a slice that holds a NaN is NaN throughout.  Host arrays give an
    array, float64 device tensors are read in place and give a tensor on the same device.  ``workspace_bytes`` bounds
    the sort's buffers for a batch of slices (0: half of the free device memory); the ranks do not depend on it."""
    if _lib.is_device_tensor(values):
        import torch
        if values.dtype != torch.float64:
            raise TypeError("device ranking needs float64 tensors")
        flat, rs, es, lead = _flat_rows(values, axis)
        if flat is None:
            raise ValueError("no elements to rank")
        R, S = flat.shape
        out = torch.empty((R, S), dtype=torch.float64, device=values.device)
        check(_lib.lib().gpemu_rank_dev(int(values.device.index or 0), R, S, C.c_void_p(flat.data_ptr()), rs, es,
                                        C.c_void_p(out.data_ptr()), int(workspace_bytes),
                                        _lib.current_stream(values.device)))
        return out.reshape(*lead, S).movedim(-1, axis)
    _lib.require_device()
    v = np.asarray(values, dtype=np.float64)
    if v.ndim == 0:
        raise ValueError("values must have at least one axis")
    v = np.moveaxis(v, axis, -1)
    S = v.shape[-1]
    lead = v.shape[:-1]
    v = np.ascontiguousarray(v).reshape(-1, S)
    if v.size == 0:
        raise ValueError("no elements to rank")
    out = np.empty_like(v)
    check(_lib.lib().gpemu_rank(int(_lib.resolve_device(device)), v.shape[0], S, ptr(v), ptr(out)))
    return np.moveaxis(out.reshape(*lead, S), -1, axis)
