"""Guards (tests only): the arena and the gate that make a kernel show which writes or reads outside the arrays it was
given (tests/test_gpu_guards.py, tests/test_guards_host.py; DESIGN.md "The guard gate").

Every device array of one call of a row of tests/stream_cases.py -- inputs, then outputs in the order the closure asks
for them -- is carved out of ONE device arena, every host output out of one host arena.  Every 64-bit word of an arena
first holds ``index * K ^ salt`` (K odd): no constant, zero or NaN a kernel might write reproduces it.  Before, between
and after the arrays lie guard bands of ``max(64 KiB, 2 x the array's bytes)`` plus one word, so an array starts 8-byte
but not 16-byte aligned: the C contract is the natural alignment of double / int64.  The 16-byte loads of k_gemm.hip,
k_trmm_small.hip, k_halfstep.hip and k_pca.hip read the library's own operands; one kernel stores 16 bytes at a time
to a caller's pointer, the matrix-core writer of gpemu_predict_full_dev (k_exact.hip), and its launcher takes the
row-wise writer where dcov is not 16-byte aligned -- other bits, as the header says.  That row (``by_alignment``) is
swept at both alignments (``Shape.a16``), against plain tensors aligned alike.  An output with a leading dimension is carved with ld > n; its padding columns belong
to the guard.  The guards never end: every array is surrounded by memory the test owns, so a short overrun lands in the
arena and is reported, it does not fault.

After a call, on a synchronised device (``Outcome.findings``, each naming row, shape, array, side and byte offset):
  a. every guard unit (4 bytes), device and host, holds its pattern;
  b. every input holds the bytes it was given;
  c. the results equal, bit for bit, those of the reference run (``SC.quiet`` with plain tensors);
  d. (c) under two fills of the guards around the inputs and of the gap rows of a view: NaN, and the row's decoy;
  e. (c) under two prefills of the outputs, NaN / -1 and 1/7 / 7; an element keeps its prefill under both exactly where
     the row's ``unwritten`` mask says so;
  f. a call that declines has written nothing since the last call of the closure that succeeded.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import stream_cases as SC

K_ODD = 0x9E3779B97F4A7C15
SALT_DEVICE, SALT_HOST = 0x5DEECE66D1CE4E5B, 0x2545F4914F6CDD1D
GUARD_MIN = 64 << 10
DEVICE_BYTES, HOST_BYTES = 24 << 20, 4 << 20
PREFILLS = {"nan": (np.nan, -1), "finite": (1.0 / 7, 7)}
BEFORE, AFTER, PADDING = "before", "after", "padding"


class Declined(Exception):
    """a stand-in entry's refusal (the library's own is GpemuError)"""

    def __init__(self, code):
        super().__init__(f"declined with {code}")
        self.code = code


def _refusals():
    try:
        from gpemu._lib import GpemuError
        return (Declined, GpemuError)
    except Exception:                     # (no library on this machine: the host self-test runs stand-ins only)
        return (Declined,)


@lru_cache(maxsize=None)
def pattern(nwords, salt):
    p = (np.arange(nwords, dtype=np.uint64) * np.uint64(K_ODD)) ^ np.uint64(salt)
    p.setflags(write=False)
    return p


@lru_cache(maxsize=None)
def _pristine(nwords, salt):
    import torch
    return torch.from_numpy(pattern(nwords, salt).view(np.int64).copy()).to(torch.device("cuda", 0))


@dataclass
class Finding:
    kind: str                             # guard | input | result | unwritten | prefill | decline
    array: str
    side: str = ""                        # before | after | padding (guards)
    offset: int = -1                      # bytes: from the array's start (padding, input, result), before its start or
    text: str = ""                        # past its end

    def __str__(self):
        return self.text


@dataclass
class Block:
    name: str
    role: str                             # input | output
    where: str                            # device | host
    shape: tuple
    dtype: np.dtype
    ld: int
    start: int                            # in 4-byte units from the arena's start
    units: int                            # of the whole region, padding included
    band: int                             # units of guard on each side
    owned: np.ndarray                     # per unit of the region: an element of the array (not padding)
    given: np.ndarray                     # the elements written when it was carved (inputs: the data; outputs: the prefill)
    view: object = None
    calls_ok: int = 0                     # SC.CALLS_OK when it was carved
    after: np.ndarray = None              # the elements after the call

    @property
    def end(self):
        return self.start + self.units + (self.units & 1)       # (the next whole word)


class Arena:
    def __init__(self, nbytes, salt, on_device, odd=True):
        self.nwords, self.on_device, self.odd = nbytes // 8, on_device, odd
        self.expect = pattern(self.nwords, salt).copy()          # what lies outside the arrays
        if on_device:
            self.buf = _pristine(self.nwords, salt).clone()
            base = self.buf.data_ptr()
        else:
            self.buf = self.expect.copy()
            base = self.buf.ctypes.data
        assert base % 16 == 0
        self.blocks, self.at, self.pending = [], 0, 0

    # ---- raw access in 4-byte units
    def _put(self, a, units):
        units = np.ascontiguousarray(units, dtype=np.uint32)
        if self.on_device:
            import torch
            self.buf.view(torch.int32)[a:a + units.size].copy_(torch.from_numpy(units.view(np.int32)))
        else:
            self.buf.view(np.uint32)[a:a + units.size] = units

    def _get(self, a, n):
        if self.on_device:
            import torch
            return self.buf.view(torch.int32)[a:a + n].cpu().numpy().view(np.uint32)
        return self.buf.view(np.uint32)[a:a + n].copy()

    def carve(self, name, role, shape, dtype, content, ld=None, guard_fill=None):
        """an array of ``shape`` (rows ``ld`` apart), its owned elements set to ``content`` (broadcast), between guards;
        ``guard_fill``: values that replace the pattern in its two guard bands"""
        dtype, shape = np.dtype(dtype), tuple(int(n) for n in shape)
        assert dtype.itemsize in (4, 8) and len(shape) >= 1 and min(shape) >= 1, (name, shape, dtype)
        n, rows = shape[-1], int(np.prod(shape[:-1], dtype=np.int64))
        ld = n if ld is None else int(ld)
        assert ld >= n and (ld == n or len(shape) == 2)
        u = dtype.itemsize // 4
        nbytes = rows * ld * dtype.itemsize
        band_w = (max(GUARD_MIN, 2 * nbytes) + 7) // 8 + 1
        start_w = self.at + max(self.pending, band_w)
        start_w += (start_w & 1) ^ self.odd                      # odd: 8-byte, not 16-byte aligned
        end_w = start_w + (nbytes + 7) // 8
        assert end_w + band_w <= self.nwords, f"{name}: the arena of {8 * self.nwords} bytes is too small"
        self.at, self.pending = end_w, band_w
        owned_el = np.zeros((rows, ld), dtype=bool)
        owned_el[:, :n] = True
        owned = np.repeat(owned_el.reshape(-1), u)
        given = np.ascontiguousarray(np.broadcast_to(np.asarray(content, dtype=dtype), shape))
        b = Block(name, role, "device" if self.on_device else "host", shape, dtype, ld, 2 * start_w, rows * ld * u, 2 * band_w,
                  owned, given, calls_ok=SC.CALLS_OK[0])
        e32 = self.expect.view(np.uint32)
        if guard_fill is not None:
            fill = np.asarray(guard_fill, dtype=dtype).reshape(-1)
            for a in (b.start - b.band, b.end):
                e32[a:a + b.band] = np.resize(fill, b.band // u).view(np.uint32)
                self._put(a, e32[a:a + b.band])
        region = e32[b.start:b.start + b.units].copy()
        region[owned] = given.reshape(-1).view(np.uint32)
        self._put(b.start, region)
        count = rows * ld
        if self.on_device:
            import torch
            tdt = {"float64": torch.float64, "int64": torch.int64, "int32": torch.int32}[dtype.name]
            flat = self.buf[start_w:end_w].view(tdt)[:count]
            b.view = flat.view(shape) if ld == n else flat.view(rows, ld)[:, :n]
            assert b.view.data_ptr() % 16 == 8 * self.odd
        else:
            flat = self.buf[start_w:end_w].view(dtype)[:count]
            b.view = flat.reshape(shape) if ld == n else flat.reshape(rows, ld)[:, :n]
            assert b.view.ctypes.data % 16 == 8 * self.odd and np.shares_memory(b.view, self.buf)
        self.blocks.append(b)
        return b

    def check(self, what):
        """reads the blocks' elements back (``Block.after``) and returns the findings of (a)"""
        used = 2 * (self.at + self.pending)
        got, want = self._get(0, used), self.expect.view(np.uint32)[:used]
        guard = np.ones(used, dtype=bool)
        for b in self.blocks:
            guard[b.start:b.start + b.units][b.owned] = False
            b.after = got[b.start:b.start + b.units][b.owned].view(b.dtype).reshape(b.shape)
        bad = np.flatnonzero((got != want) & guard)
        first, count = {}, {}
        for i in bad[:4096]:
            b, side, off = self._classify(int(i))
            first.setdefault((b.name, side), (int(i), b, off))
            count[b.name, side] = count.get((b.name, side), 0) + 1
        found = []
        for (_, side), (i, b, off) in first.items():
            n = count[b.name, side] if bad.size <= 4096 else f"{bad.size} in all;"
            where = {BEFORE: f"{off} bytes before its start", AFTER: f"{off} bytes past its end",
                     PADDING: f"in its padding (ld = {b.ld}), {off} bytes from its start"}[side]
            found.append(Finding("guard", b.name, side, off, f"{what}: the {b.where} guard {side} {b.role} '{b.name}' "
                                 f"{b.shape} was written: first {where} ({n} units of 4 bytes differ; holds "
                                 f"{got[i]:#010x}, the pattern is {want[i]:#010x})"))
        return found

    def _classify(self, i):
        for b in self.blocks:
            if b.start <= i < b.start + b.units:
                return b, PADDING, 4 * (i - b.start)
        best = None
        for b in self.blocks:
            for side, dist, off in ((BEFORE, b.start - i, 4 * (b.start - i)),
                                    (AFTER, i - (b.start + b.units) + 1, 4 * (i - (b.start + b.units)))):
                if dist > 0 and (best is None or dist < best[0]):
                    best = (dist, b, side, off)
        return best[1:]


# ---- the allocators a closure sees ------------------------------------------------------------------------------------
class GuardOuts:
    """``out(shape, dtype, ld)`` / ``out.host(shape, dtype)`` of a closure of tests/stream_cases.py, carving from the arenas"""

    def __init__(self, dev, host, prefill):
        self.dev, self.host_arena, self.prefill = dev, host, PREFILLS[prefill]
        self.made, self.blocks = [], []

    def _fill(self, dtype):
        return self.prefill[0] if np.dtype(dtype).kind == "f" else self.prefill[1]

    def __call__(self, shape, dtype=None, ld=None):
        if dtype is None:
            dtype = np.float64
        dtype = np.dtype(str(dtype).replace("torch.", "") if hasattr(dtype, "is_floating_point") else dtype)
        b = self.dev.carve(f"out{len(self.blocks)}", "output", shape, dtype, self._fill(dtype), ld=ld)
        self.blocks.append(b)
        self.made.append(b.view)
        return b.view

    def host(self, shape, dtype=np.float64):
        b = self.host_arena.carve(f"out{len(self.blocks)}(host)", "output", shape, dtype, self._fill(dtype))
        self.blocks.append(b)
        return b.view


class PlainOuts:
    """the same interface with arrays of their own (the reference of a stand-in entry on the host)"""

    def __init__(self):
        self.made = []

    def __call__(self, shape, dtype=None, ld=None):
        if ld is None:
            return SC.Outs.host(self, shape, dtype or np.float64)
        return SC.Outs.host(self, (shape[0], ld), dtype or np.float64)[:, :shape[1]]

    host = SC.Outs.host


@dataclass
class Outcome:
    declined: object                      # None, or the error code
    res: tuple                            # the results as host arrays (empty after a decline)
    findings: list
    outs: list = field(default_factory=list)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _first_diff(a, b):
    bad = np.flatnonzero((_bits(a) != _bits(b)).reshape(-1))
    return bad.size, (int(bad[0]) if bad.size else -1)


def _sync(on_device):
    if on_device:
        import torch
        torch.cuda.synchronize()


def guarded(row, P, dm, inputs, what, prefill="nan", fill=None, decoy=None, on_device=True):
    """One call of ``row.run`` with every array carved from the arenas.  ``fill``: None (the guards hold the pattern),
    "nan" or "decoy" (the guards of the inputs, and the gap rows of the row's views, hold NaN / -1 or ``decoy``)."""
    dev = Arena(DEVICE_BYTES if on_device else HOST_BYTES, SALT_DEVICE, on_device, odd=not SC.A16)
    host = Arena(HOST_BYTES, SALT_HOST, False)
    T, ins = {}, []
    for name, a in inputs.items():
        a = np.array(a, copy=True)
        gf = None
        if fill is not None:
            gf = decoy[name] if fill == "decoy" else (np.nan if a.dtype.kind == "f" else -1)
            if name in row.gaps:
                m = SC.gap_mask(a.shape)
                a[m] = np.resize(np.asarray(gf, dtype=a.dtype).reshape(-1), int(m.sum()))
        b = dev.carve(name, "input", a.shape, a.dtype, a, guard_fill=gf)
        T[name] = b.view
        ins.append(b)
    out = GuardOuts(dev, host, prefill)
    _sync(on_device)
    declined, res = None, ()
    try:
        res = row.run(0, T, out, P, dm)
        _sync(on_device)
        res = tuple(np.array(r if isinstance(r, np.ndarray) else r.cpu().numpy(), copy=True) for r in res)
    except _refusals() as e:
        declined = e.code
        _sync(on_device)
    found = dev.check(what) + host.check(what)
    for b in ins:                                                # (b)
        n, i = _first_diff(b.after, b.given)
        if n:
            found.append(Finding("input", b.name, "", i * b.dtype.itemsize,
                                 f"{what}: input '{b.name}' {b.shape} was written: {n} elements differ, first at byte "
                                 f"{i * b.dtype.itemsize} (element {i}): holds {b.after.reshape(-1)[i]!r}, was given "
                                 f"{b.given.reshape(-1)[i]!r}"))
    if declined is not None:                                     # (f)
        for b in out.blocks:
            n, i = _first_diff(b.after, b.given)
            if n and b.calls_ok == SC.CALLS_OK[0]:
                found.append(Finding("decline", b.name, "", i * b.dtype.itemsize,
                                     f"{what}: declined with {declined} after writing output '{b.name}' {b.shape}: {n} "
                                     f"elements, first at byte {i * b.dtype.itemsize}"))
    return Outcome(declined, res, found, out.blocks)


def reference_host(row, inputs):
    """a stand-in entry with plain host arrays: ('ok', results) or ('declined', code)"""
    try:
        return ("ok", tuple(np.array(r, copy=True) for r in
                            row.run(0, {k: np.array(v, copy=True) for k, v in inputs.items()}, PlainOuts(), None, None)))
    except Declined as e:
        return ("declined", e.code)


def reference_device(row, P, dm, inputs):
    """``SC.quiet``: plain tensors of their own, on a quiet device (for a row that picks a launch path by the alignment
    of an output, the outputs aligned as the arena's are)"""
    try:
        return ("ok", SC.quiet(row, P, dm, inputs, odd=row.by_alignment and not SC.A16)[0])
    except _refusals() as e:
        return ("declined", e.code)


def against(what, o, want):
    """(c): the results of a guarded call against the reference's"""
    if want[0] == "declined" or o.declined is not None:
        if (o.declined is not None) != (want[0] == "declined") or (o.declined is not None and o.declined != want[1]):
            return [Finding("result", "", text=f"{what}: {'declined with ' + str(o.declined) if o.declined is not None else 'ran'}"
                            f" in the arena, the reference {'declined with ' + str(want[1]) if want[0] == 'declined' else 'ran'}")]
        return []
    got, ref = o.res, want[1]
    if len(got) != len(ref) or not ref:
        return [Finding("result", "", text=f"{what}: {len(got)} results, the reference has {len(ref)}")]
    found = []
    for k, (a, b) in enumerate(zip(got, ref)):
        if a.shape != b.shape or a.dtype != b.dtype:
            found.append(Finding("result", f"result{k}", text=f"{what}: result {k} is {a.dtype}{a.shape}, the reference's {b.dtype}{b.shape}"))
            continue
        n, i = _first_diff(a, b)
        if n:
            found.append(Finding("result", f"result{k}", "", i * a.dtype.itemsize,
                                 f"{what}: result {k} {a.shape} differs from the reference's in {n} elements, first at byte "
                                 f"{i * a.dtype.itemsize} (element {i}): {a.reshape(-1)[i]!r}, the reference has "
                                 f"{b.reshape(-1)[i]!r}"))
    return found


def prefill_findings(what, row, A, B):
    """(e): an element of an output either holds the same bits under both prefills, or keeps its prefill under both --
    the latter exactly where ``row.unwritten(k, shape)`` says so"""
    found = []
    if A.declined is not None or B.declined is not None:
        return found
    assert len(A.outs) == len(B.outs)
    for k, (a, b) in enumerate(zip(A.outs, B.outs)):
        kept = (_bits(a.after) == _bits(a.given)) & (_bits(b.after) == _bits(b.given))
        same = _bits(a.after) == _bits(b.after)
        declared = row.unwritten(k, a.shape) if row.unwritten is not None else None
        declared = np.zeros(a.shape, dtype=bool) if declared is None else np.broadcast_to(declared, a.shape)
        for mask, kind, text in ((~same & ~kept, "prefill", "depend on what the output held before"),
                                 (kept & ~declared, "unwritten", "were left unwritten, which the row does not declare"),
                                 (declared & ~kept, "unwritten", "were written, though the row declares them unwritten")):
            bad = np.flatnonzero(mask.reshape(-1))
            if bad.size:
                i = int(bad[0])
                found.append(Finding(kind, a.name, "", i * a.dtype.itemsize,
                                     f"{what}: {bad.size} elements of output '{a.name}' {a.shape} {text}, first at byte "
                                     f"{i * a.dtype.itemsize} (element {i}): {a.after.reshape(-1)[i]!r} after a prefill of "
                                     f"{a.given.reshape(-1)[i]!r}, {b.after.reshape(-1)[i]!r} after {b.given.reshape(-1)[i]!r}"))
    return found


def gate_outputs(row, P, dm, inputs, what, want, on_device=True):
    """(a)-(c), (e), (f): (declined code or None, findings)"""
    A = guarded(row, P, dm, inputs, f"{what} [prefill NaN/-1]", "nan", on_device=on_device)
    B = guarded(row, P, dm, inputs, f"{what} [prefill 1/7, 7]", "finite", on_device=on_device)
    found = A.findings + B.findings + against(f"{what} [prefill NaN/-1]", A, want) + against(f"{what} [prefill 1/7, 7]", B, want)
    return A.declined, found + prefill_findings(what, row, A, B)


def gate_input_guards(row, P, dm, inputs, decoy, what, want, on_device=True):
    """(d), with (a) and (b): the guards of the inputs hold NaN, then the decoy"""
    found = []
    for fill in ("nan", "decoy"):
        o = guarded(row, P, dm, inputs, f"{what} [input guards: {fill}]", "nan", fill=fill, decoy=decoy, on_device=on_device)
        found += o.findings + against(f"{what} [input guards: {fill}]", o, want)
    return o.declined, found


def report(found):
    assert not found, f"{len(found)} findings:\n" + "\n".join(str(f) for f in found)


# ---- the sweep ----------------------------------------------------------------------------------------------------------
FAMILIES = (SC.MODEL_BOUND, SC.DEVICE_WIDE, SC.HANDLE_CREATING, SC.SAMPLER_COMM)
GUARD_CASES = None                        # the problems of a model-bound row the sweep runs on: all (a number: the first)


def sweep():
    """(row, case, shape) of the guard sweep"""
    return [(r, c, sh) for r, c in SC.sweep_params(FAMILIES) if c is None or c in r.cases[:GUARD_CASES] for sh in r.edge_shapes]


def padded_sweep():
    """(row, case, shape) of the rows with an output's leading dimension, at both paddings, at three of their shapes"""
    import dataclasses
    return [(r, c, dataclasses.replace(sh, pad=pad)) for r, c in SC.sweep_params(FAMILIES) if r.out_ld
            if c is None or c in r.cases[:GUARD_CASES] for sh in r.edge_shapes[1::3] for pad in SC.PADS]


def sweep_id(rcs):
    return f"{SC.param_id(rcs[:2])}-{rcs[2]}"


# ---- host-side pokes for the stand-in entries of tests/test_guards_host.py -------------------------------------------------
def poke(address, value):
    C.c_double.from_address(address).value = value


def peek(address):
    return C.c_double.from_address(address).value
