"""Streams (tests only): the table of every entry point of include/gpemu.h that takes a ``void *stream`` or carries one
in a ``const gpemu_call_ctx *``, and the gate that makes a launch on the wrong stream show, whatever the timing
(tests/test_gpu_streams.py, tests/test_streams_host.py).

A row names the entry, its family, the header's own words on what NULL means for it and on whether it waits, and a
closure ``run(st, T, out, P, dm) -> tuple`` that calls it at a small shape -- the module's constants, which ``shaped``
rebinds to a ``Shape`` for the guard sweep of tests/guard_cases.py: ``st`` the ``void *`` to pass, ``T``
the device inputs (torch tensors by name, as ``inputs(P, seed)`` made them), ``out(shape, dtype, ld)`` the allocator of
the device outputs and ``out.host(shape, dtype)`` of the host outputs, ``P`` / ``dm`` the problem of tests/reuse_cases.py and its model handle (None for the device-wide rows).
The closure returns device tensors (read on the stream under test) and host arrays.

The gate (``gated``): the device inputs hold a decoy -- finite, in-box, valid values of another seed -- and the outputs
NaN (integers: -1).  On the stream under test ``s`` go ``torch.cuda._sleep(cycles)`` and then the asynchronous copies of
the true inputs over the decoys; the call follows under ``torch.cuda.stream(s)`` with ``s.cuda_stream``; the outputs
are cloned on ``s`` and read after ``s.synchronize()``.  A launch, fill or copy of the library on any other stream reads
the decoy or lands under the copies; work that is not ordered after the call's does not see its results.  ``s.query()``
must be False right before the call (the gate was still closed) and, for an entry documented not to wait, right after
it; a run that misses either fails with its own message.  ``differs`` is the other half: the same call on the
decoy, on a quiet device, gives other bytes.

Gate length.  ``calibrate`` times one ``_sleep`` with torch events, once per session.  Measured on an MI355X (this
file's tests, one session): 1e6 cycles of ``_sleep`` take 0.4179 ms (GATE_CALIBRATION_MS_PER_MCYCLE); the longest host
time from enqueueing the gate to the return of a call that does not wait (to the entry of one that waits) was 6.821 ms
(GATE_LONGEST_HOST_MS: the first gated call of the session; 0.33 ms at most for every later one, over all rows).
GATE_MS, 70 ms, is ten times that, and no more than 200 ms.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import time
from contextlib import contextmanager
import dataclasses
from dataclasses import dataclass

import numpy as np

import reuse_cases as R

# measured, see the docstring (the gate's conditions keep a too-short gate from passing silently)
GATE_CALIBRATION_MS_PER_MCYCLE = 0.4179
GATE_LONGEST_HOST_MS = 6.821             # the first gated call of a session (gpemu_gp_predict_dev); 0.33 ms after it
GATE_MS = 70.0

S_WIDE = 257                              # one past the 256-row tiles of the device-wide entries
D_WIDE = 3
VIEW = (16, 4, 6)                         # a chain view: 16 steps x 4 walkers, steps 6 rows apart
B_SMALL, B_BIG = 33, 130                  # at and just past the tile and half-step limits of the launch paths

M2_COV = 17                               # gpemu_gp_predict_cov_dev: the columns of the rectangular call
A16 = False                               # the guard arena: arrays 16-byte aligned (else 8-byte, not 16-byte)
PAD = 0                                   # what an output's leading dimension exceeds its row length by (the guard sweep)



@dataclass(frozen=True)
class Shape:
    """The sizes the closures of this table are called at.  The defaults are the module's constants above: what the
    stream, allocation and reuse gates run.  ``shaped(sh)`` rebinds the constants for the guard sweep of
    tests/guard_cases.py, which calls every row at the ``edge_shapes`` beside it."""
    S: int = S_WIDE
    D: int = D_WIDE
    VIEW: tuple = VIEW
    B_SMALL: int = B_SMALL
    B_BIG: int = B_BIG
    RW: int = 2
    M2: int = M2_COV
    pad: int = PAD
    a16: bool = A16

    def __str__(self):
        d = Shape()
        diff = [f"{k}={getattr(self, k)}" for k in self.__dataclass_fields__ if getattr(self, k) != getattr(d, k)]
        return ",".join(diff).replace(" ", "") or "default"


# ---- the edge shapes of the guard sweep: one below, at and one above every tile, chunk and wave size of the kernels ---
def _S(*sizes, **kw):
    return tuple(Shape(S=s, **kw) for s in sizes)


# a wave (64 lanes), the 256-thread workgroups and 256-row tiles of the device-wide kernels (rows_dev.h RK_BINS /
# SEL_BINS, k_knn.hip's 256-query tiles, GPEMU_KNN_REF_TILE), and d = 1, 3 (the default), 16 = the widest row
S_EDGES = _S(1, 2, 63, 64, 65, 255, 256, 257)
D_EDGES = (Shape(S=65, D=1), Shape(S=65, D=16), Shape(S=257, D=16))
# the radix sort and select work on 2048 keys per workgroup (rows_dev.h RK_TILE; k_marginal.hip WH_SCAN, the weighted
# HPD's prefix sum; GPEMU_PAIRLSE_CHUNK columns of Z)
S_CHUNK_2048 = _S(2047, 2048, 2049)
# partial sums over 4096 samples (k_loo.hip LOO_SUM, k_reweight.hip RW_SUM, rows_dev.h WS_SUM, k_select.hip SEL_SLICE,
# k_marginal.hip HW_PER windows)
S_CHUNK_4096 = _S(4095, 4096, 4097)
# 8192 samples per partial sum of the densities (k_marginal.hip KD_CHUNK, k_kde2d.hip K2_CHUNK), staged 1024 at a time
# (KD_STAGE); rows_dev.h MOM_ROWS and k_knn.hip LS_ROWS = 1024 rows per partial of the moments and the log sums
S_CHUNK_1024 = _S(1023, 1024, 1025)
S_CHUNK_8192 = _S(8191, 8192, 8193)
# rows of a model: the 32-row cross-kernel form and KSTAR_SMALL_MAX = 128 (internal.h), TM = 64 rows per item
# (sched_host.h), TILE = 128, PC_NB = 64 (pcov_dev.h), k_design.hip T = 64: tests/reuse_cases.py LOGPOST_B is the precedent
B_EDGES = tuple(Shape(B_SMALL=b, B_BIG=b) for b in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129))
# gpemu_gp_predict_cov_dev: M2 = 1, below, at and above M1, on both sides of PC_NB = 64 (pcov_dev.h)
PCOV_EDGES = tuple(Shape(B_SMALL=m1, B_BIG=m1, M2=m2) for m1, m2 in
                   ((1, 1), (31, 33), (32, 32), (33, 1), (33, 32), (63, 65), (64, 64), (65, 63), (65, 1), (127, 129),
                    (128, 128), (129, 127)))
# views: contiguous, nb*br no multiple of 64 (a wave), today's, and one of 68 rows with gaps of 5 rows between the blocks
VIEW_EDGES = tuple(Shape(VIEW=v) for v in ((1, 1, 1), (3, 5, 5), (16, 4, 6), (17, 4, 9)))
WIDE_S = S_EDGES + D_EDGES
WIDE_V = S_EDGES                          # (rows that take value rows V and no d)
PADS = (1, 7)                             # ld = n + 1 and n + 7: the paddings of the outputs with a leading dimension


MODEL_BOUND, DEVICE_WIDE, HANDLE_CREATING, SAMPLER_COMM = "model-bound", "device-wide", "handle-creating", "sampler/comm"

# What NULL means and whether the entry waits, in the header's own words.  (quote, where): the quote must stand in the
# Conventions block at the top of include/gpemu.h ("conventions") or in the section of the prototype ("section").
NULL_MODEL = "NULL = the model's"
NULL_NULL = "NULL = the null stream"
NULL_NONE = "NULL: none"
NULL_FIRST_GROUP = "NULL = the first group's stream"
NOWAIT = "do not synchronise"
WAITS = "waits for it"


# ---- include/gpemu.h as the CPU gates read it (tests/test_streams_host.py, tests/test_devmem_tables_host.py) -------------
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpemu.h")
STREAM_PARAM = r"\bvoid\s*\*\s*stream\b"
CTX_PARAM = r"\bconst\s+gpemu_call_ctx\s*\*"


def header_text():
    with open(HEADER) as f:
        return f.read()


def all_prototypes(text):
    """{name: (offset, parameter list)} of every function prototype of the header"""
    code = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)      # comments blanked, offsets kept
    return {m.group(1): (m.start(), m.group(2))
            for m in re.finditer(r"\b(?:int|void|int64_t)\s+(gpemu_\w+)\s*\(([^;{]*?)\)\s*;", code)}


def prototypes_with(text, pattern):
    """{name: offset} of the prototypes whose parameter list matches `pattern`"""
    return {name: at for name, (at, params) in all_prototypes(text).items() if re.search(pattern, params)}


def stream_prototypes(text):
    """{name: offset} of every function prototype with a ``void *stream`` or a ``const gpemu_call_ctx *`` parameter"""
    return prototypes_with(text, f"{STREAM_PARAM}|{CTX_PARAM}")


@dataclass
class Row:
    name: str
    family: str
    null_means: str                       # one of the NULL_* quotes
    waits: bool
    doc: tuple                            # the quotes of the header that say so: ((quote, "conventions" | "section"), ...)
    inputs: object = None                 # (P, seed) -> {name: numpy array}: the DEVICE inputs
    run: object = None                    # (st, T, out, P, dm) -> tuple of device tensors and host arrays
    cases: tuple = ()                     # model-bound: the problems of reuse_cases it runs on
    omitted: str = ""                     # why the GPU sweep leaves it out
    edge_shapes: tuple = ()               # the Shapes of the guard sweep (tests/guard_cases.py), beside today's
    out_ld: tuple = ()                    # the ld* / stride parameters of the prototype that belong to an OUTPUT
    gaps: tuple = ()                      # the inputs that are rows of a VIEW: the rows between its blocks are not read
    by_alignment: bool = False            # it picks a launch path by the 16-byte alignment of an output: swept at both
    unwritten: object = None              # (k, shape) -> mask of the elements of the k-th output the header says stay


def _vp(x):
    """a device tensor, an address or a host array as ``void *`` (None / 0: NULL)"""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data_as(C.c_void_p)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x)) if int(x) else None


def _L():
    from gpemu import _lib
    return _lib.lib()


CALLS_OK = [0]                            # the library calls of the closures that returned GPEMU_OK so far


def _ck(code):
    from gpemu import _lib
    _lib.check(code)
    CALLS_OK[0] += 1


def _rng(seed, tag):
    import zlib
    return np.random.default_rng([int(seed), zlib.crc32(tag.encode())])


i64 = lambda *v: np.ascontiguousarray(np.array(v, dtype=np.int64).reshape(-1))
f64 = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.float64))


# ---- device-wide rows: S_WIDE rows of D_WIDE parameters in the unit box -----------------------------------------------
def _unit_rows(seed, tag, n=None, d=None, lo=0.1):
    return _rng(seed, tag).uniform(lo, 1.0, (S_WIDE if n is None else n, D_WIDE if d is None else d))


def _in_X(P, seed):
    return {"X": _unit_rows(seed, "X")}


def _in_V(P, seed):
    """R = 3 rows of S values (the parameters of the rows above, one parameter per row)"""
    return {"V": np.ascontiguousarray(_unit_rows(seed, "V", d=3).T)}


def _in_view(P, seed):
    nb, br, bs = VIEW
    return {"X": _unit_rows(seed, "view", nb * bs)}


def _edges(nb, d):
    return np.ascontiguousarray(np.tile(np.linspace(0.0, 1.0, nb + 1), (d, 1)))


EDGES1, EDGES2 = _edges(8, D_WIDE), _edges(4, D_WIDE)


def _n_pairs():
    return D_WIDE * (D_WIDE - 1) // 2


def _fixed_weights(g, rows, n, log2_total):
    """rows of n integer weights whose total lies in [2^log2_total, 2^(log2_total + 1)) whatever the seed and n: drawn
    from [lo, 2 lo) with lo = 2^log2_total / 2^floor(log2 n), and halved where the total reaches the upper end"""
    lo = 2 ** (log2_total - (int(n).bit_length() - 1))
    q = g.integers(lo, 2 * lo, (rows, n)).astype(np.int64)
    q[q.sum(axis=1) >= 2 ** (log2_total + 1)] >>= 1
    return q


def _select(st, T, out, P, dm):
    ranks = i64(0, S_WIDE // 2, S_WIDE - 1)
    o = out((3, 3))
    _ck(_L().gpemu_select_dev(0, 3, S_WIDE, _vp(T["V"]), S_WIDE, 1, 3, _vp(ranks), _vp(o), _vp(st)))
    return (o,)


def _rank(st, T, out, P, dm):
    o = out((3, S_WIDE))
    _ck(_L().gpemu_rank_dev(0, 3, S_WIDE, _vp(T["V"]), S_WIDE, 1, _vp(o), 0, _vp(st)))
    return (o,)


def _hist(st, T, out, P, dm):
    import torch
    h1 = out((D_WIDE, 8), torch.int64)
    h2 = out((_n_pairs(), 4, 4), torch.int64) if D_WIDE > 1 else None          # (NULL allowed for d = 1)
    ni = out((D_WIDE,), torch.int64)
    _ck(_L().gpemu_marginal_hist_dev(0, _vp(T["X"]), 1, S_WIDE, S_WIDE, D_WIDE, 8, _vp(EDGES1), 4, _vp(EDGES2), 0,
                                     _vp(h1), _vp(h2), _vp(ni), _vp(st)))
    return tuple(a for a in (h1, h2, ni) if a is not None)


def _hpd(st, T, out, P, dm):
    n_out = i64(max(1, (S_WIDE + 5) // 10), 1)
    o = out((3, 2, 2))
    _ck(_L().gpemu_hpd_dev(0, 3, S_WIDE, _vp(T["V"]), S_WIDE, 1, 2, _vp(n_out), _vp(o), 0, _vp(st)))
    return (o,)


def _kde1d(st, T, out, P, dm):
    G = 16
    grid = np.ascontiguousarray(np.tile(np.linspace(0.0, 1.0, G), (3, 1)))
    h = f64([0.05, 0.07, 0.09])
    o = out((3, G))
    _ck(_L().gpemu_kde1d_dev(0, 3, S_WIDE, _vp(T["V"]), S_WIDE, 1, G, _vp(grid), _vp(h), _vp(o), _vp(st)))
    return (o,)


def _dense(st, T, out, P, dm):
    nb, br, bs = VIEW
    o = out((nb * br, D_WIDE))
    _ck(_L().gpemu_marginal_dense_dev(0, _vp(T["X"]), nb, br, bs, D_WIDE, _vp(o), _vp(st)))
    return (o,)


def _moments(st, T, out, P, dm):
    mean, var = out.host((D_WIDE,)), out.host((D_WIDE,))
    _ck(_L().gpemu_marginal_moments_dev(0, _vp(T["X"]), S_WIDE, D_WIDE, _vp(mean), _vp(var), _vp(st)))
    return mean, var


_SHEAR = f64([0.1, -0.2])


def _pairs():
    """(0, 1) and (d - 1, 0); with d = 1 there is no pair, and the entries decline"""
    return i64(0, 1, D_WIDE - 1, 0)


def _kde2d(st, T, out, P, dm):
    G = 16
    bw = f64([0.1, 0.12, 0.08, 0.1])
    ga = np.ascontiguousarray(np.tile(np.linspace(0.0, 1.0, G), (2, 1)))
    gb = np.ascontiguousarray(np.tile(np.linspace(-0.2, 1.2, G), (2, 1)))
    o = out((2, G, G))
    _ck(_L().gpemu_kde2d_dev(0, _vp(T["X"]), 1, S_WIDE, S_WIDE, D_WIDE, 2, _vp(_pairs()), _vp(_SHEAR), _vp(bw), G, _vp(ga),
                             _vp(gb), _vp(o), 0, _vp(st)))
    return (o,)


def _pair_moments(st, T, out, P, dm):
    mean, cov, ext = out.host((D_WIDE,)), out.host((D_WIDE, D_WIDE)), out.host((2, 2))
    _ck(_L().gpemu_pair_moments_dev(0, _vp(T["X"]), 1, S_WIDE, S_WIDE, D_WIDE, _vp(mean), _vp(cov), 2, _vp(_pairs()),
                                    _vp(_SHEAR), _vp(ext), _vp(st)))
    return mean, cov, ext


def _in_loglik_rows(P, seed):
    """R = 3 rows of S log-likelihood values"""
    return {"V": -0.5 * _rng(seed, "loglik").normal(size=(3, S_WIDE)) ** 2 - 1.0}


def _psis(st, T, out, P, dm):
    o, lw = out((3, 9)), out((3, S_WIDE))
    _ck(_L().gpemu_psis_dev(0, 3, S_WIDE, _vp(T["V"]), S_WIDE, 1, None, _vp(o), _vp(lw), 0, _vp(st)))
    return o, lw


def _normalised(x):
    m = x.max(axis=1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))


def _in_X_logw(P, seed):
    return {"X": _unit_rows(seed, "X"), "lw": _normalised(_rng(seed, "lw").normal(size=(2, S_WIDE)))}


def _weighted_moments(st, T, out, P, dm):
    mean, var = out((2, D_WIDE)), out((2, D_WIDE))
    _ck(_L().gpemu_weighted_moments_dev(0, _vp(T["X"]), 1, S_WIDE, S_WIDE, D_WIDE, 2, _vp(T["lw"]), S_WIDE, _vp(mean),
                                        _vp(var), _vp(st)))
    return mean, var


def _group_rows(st, T, out, P, dm):
    o = out((2, S_WIDE), ld=S_WIDE + PAD)
    _ck(_L().gpemu_loo_group_rows_dev(0, 3, S_WIDE, _vp(T["V"]), S_WIDE, 2, _vp(i64(0, 2, 3)), _vp(i64(0, 1, 2)), _vp(o),
                                      S_WIDE + PAD, _vp(st)))
    return (o,)


def _unit(st, T, out, P, dm):
    lo, hi = f64(0.05 * np.arange(D_WIDE)), f64(1.0 + 0.5 * np.arange(D_WIDE))
    o = out((S_WIDE, D_WIDE))
    skipped = out.host((1,), np.int64)
    _ck(_L().gpemu_unit_rows_dev(0, _vp(T["X"]), 1, S_WIDE, S_WIDE * D_WIDE, D_WIDE, _vp(lo), _vp(hi), S_WIDE, _vp(o),
                                 skipped.ctypes.data_as(C.POINTER(C.c_int64)), _vp(st)))
    return o, skipped


def _knn_dist(st, T, out, P, dm):
    import torch
    masks = np.array([(1 << min(D_WIDE, 3)) - 1, 0b001], dtype=np.uint32)
    r2, zeros = out((2, S_WIDE)), out((2, S_WIDE), torch.int32)
    _ck(_L().gpemu_knn_dist_dev(0, S_WIDE, S_WIDE, D_WIDE, _vp(T["X"]), None, 2, _vp(masks), 4, 0, 0, _vp(r2), _vp(zeros),
                                _vp(st)))
    return r2, zeros


def _in_r2(P, seed):
    g = _rng(seed, "r2")
    return {"r2": g.uniform(1e-4, 1e-1, (2, S_WIDE)), "zeros": g.integers(0, 3, (2, S_WIDE)).astype(np.int32)}


def _knn_logsum(st, T, out, P, dm):
    counts, sums = out.host((6,), np.int64), out.host((4,))
    _ck(_L().gpemu_knn_logsum_dev(0, 2, S_WIDE, _vp(T["r2"]), _vp(T["zeros"]), None, _vp(counts), _vp(sums), _vp(st)))
    return counts, sums


def _in_YZ(P, seed):
    g = _rng(seed, "YZ")
    return {"Y": g.normal(size=(B_SMALL, 5)), "Z": g.normal(size=(S_WIDE, 5))}


def _pair_lse(st, T, out, P, dm):
    lse, ess = out((B_SMALL,)), out((B_SMALL,))
    _ck(_L().gpemu_pair_lse_dev(0, B_SMALL, S_WIDE, 5, _vp(T["Y"]), 5, _vp(T["Z"]), 5, None, None, 0, _vp(lse), _vp(ess),
                                _vp(st)))
    return lse, ess


def _centre(st, T, out, P, dm):
    o = out((5,))
    _ck(_L().gpemu_pairlse_centre_dev(0, S_WIDE, 5, _vp(T["Z"]), 5, _vp(o), _vp(st)))
    return (o,)


def _logprior(st, T, out, P, dm):
    kind = np.ascontiguousarray(np.array([[0, 1, 2], [3, 2, 0]], dtype=np.int32)[:, np.arange(D_WIDE) % 3])
    a, b, lower = np.full((2, D_WIDE), 0.5), np.full((2, D_WIDE), 0.3), np.full(D_WIDE, 0.1)
    o = out((2, S_WIDE), ld=S_WIDE + PAD)
    _ck(_L().gpemu_logprior_dev(0, _vp(T["X"]), 1, S_WIDE, S_WIDE, D_WIDE, 2, _vp(kind), _vp(a), _vp(b), _vp(lower), _vp(o),
                                S_WIDE + PAD, _vp(st)))
    return (o,)


def _in_L(P, seed):
    return {"L": _rng(seed, "L").normal(size=(2, S_WIDE))}


def _logmeanexp(st, T, out, P, dm):
    lme, lw = out((2,)), out((2, S_WIDE))
    _ck(_L().gpemu_logmeanexp_dev(0, 2, S_WIDE, _vp(T["L"]), S_WIDE, _vp(lme), _vp(lw), _vp(st)))
    return lme, lw


def _in_lw(P, seed):
    return {"lw": _normalised(_rng(seed, "lw").normal(size=(2, S_WIDE)))}


def _weights_fixed(st, T, out, P, dm):
    import torch
    q, Q = out((2, S_WIDE), torch.int64, ld=S_WIDE + PAD), out((2,), torch.int64)
    _ck(_L().gpemu_weights_fixed_dev(0, 2, S_WIDE, _vp(T["lw"]), S_WIDE, _vp(q), S_WIDE + PAD, _vp(Q), _vp(st)))
    return q, Q


def _in_Vq(P, seed):
    """values and fixed-point weights (at S = 257 in [2^39, 2^40)): a row's total lies in [2^47, 2^48) whatever the
    seed and S"""
    q = _fixed_weights(_rng(seed, "q"), 1, S_WIDE, 47)
    return {"V": np.ascontiguousarray(_unit_rows(seed, "V", d=3).T), "X": _unit_rows(seed, "X"), "q": q}


def _weighted_select(st, T, out, P, dm):
    targets = np.array([1, 2 ** 45, 2 ** 47], dtype=np.uint64)
    o = out((1, 3, 3))
    _ck(_L().gpemu_weighted_select_dev(0, 3, S_WIDE, _vp(T["V"]), S_WIDE, 1, 1, _vp(T["q"]), S_WIDE, 3, _vp(targets), _vp(o),
                                       0, _vp(st)))
    return (o,)


def _weighted_hist(st, T, out, P, dm):
    import torch
    h1 = out((1, D_WIDE, 8), torch.int64)
    h2 = out((1, _n_pairs(), 4, 4), torch.int64) if D_WIDE > 1 else None       # (NULL allowed for d = 1)
    wi = out((1, D_WIDE), torch.int64)
    _ck(_L().gpemu_weighted_hist_dev(0, _vp(T["X"]), 1, S_WIDE, S_WIDE, D_WIDE, 1, _vp(T["q"]), S_WIDE, 8, _vp(EDGES1), 4,
                                     _vp(EDGES2), 0, _vp(h1), _vp(h2), _vp(wi), _vp(st)))
    return tuple(a for a in (h1, h2, wi) if a is not None)


# the weighted chain summaries take their stream in a ``gpemu_call_ctx``; a run is built from a
# ``ctx_of(st)`` that gives the ctx to pass by reference, or None for ``ctx == NULL`` (tests/test_gpu_wsummary_streams.py)
RW2 = 2                                   # weight rows: the per-weight-row loops run twice


def ctx_on(st):
    from gpemu import _lib
    return _lib.CallCtx(int(st) or None, 0)


def _ctx_ref(ctx_of, st):
    ctx = ctx_of(st)
    return ctx, (None if ctx is None else C.byref(ctx))        # (the ctx is kept alive over the call)


def _in_Vq2(P, seed):
    """3 value rows and RW2 rows of fixed-point weights (at S = 257 in [2^39, 2^40)): a row's total lies in
    [2^47, 2^48)"""
    q = _fixed_weights(_rng(seed, "wq"), RW2, S_WIDE, 47)
    return {"V": np.ascontiguousarray(_unit_rows(seed, "wV", d=3).T), "q": q}


def _w_tables(rw):
    """per weight row: the targets of the device-wide rows, the grids and bandwidths, the targets of the view rows"""
    return (np.ascontiguousarray(np.tile(np.array([1, 2 ** 45, 2 ** 47], dtype=np.uint64), (rw, 1))),
            np.ascontiguousarray(np.tile(np.linspace(0.0, 1.1, 9), (rw * 3, 1))), np.full(rw * 3, 0.05),
            np.ascontiguousarray(np.tile(np.array([1, 2 ** 44, 2 ** 45], dtype=np.uint64), (rw, 1))))


_W_TARGETS, _W_GRID, _W_H, _W_VIEW_TARGETS = _w_tables(RW2)


def weighted_hpd_run(ctx_of):
    def run(st, T, out, P, dm):
        o = out((RW2, 3, 3, 2))
        ctx, ref = _ctx_ref(ctx_of, st)
        _ck(_L().gpemu_weighted_hpd_dev(0, 3, S_WIDE, _vp(T["V"]), S_WIDE, 1, RW2, _vp(T["q"]), S_WIDE, 3, _vp(_W_TARGETS),
                                        _vp(o), ref))
        return (o,)
    return run


def weighted_kde_run(ctx_of):
    def run(st, T, out, P, dm):
        o = out((RW2, 3, 9))
        ctx, ref = _ctx_ref(ctx_of, st)
        _ck(_L().gpemu_weighted_kde1d_dev(0, 3, S_WIDE, _vp(T["V"]), S_WIDE, 1, RW2, _vp(T["q"]), S_WIDE, 9, _vp(_W_GRID),
                                          _vp(_W_H), _vp(o), ref))
        return (o,)
    return run


def _in_chain(P, seed):
    nb, br, _ = VIEW
    return {"chain": _unit_rows(seed, "chain", nb * br).reshape(nb, br, D_WIDE)}


def _diag_create(st, T, out, P, dm):
    """the handle created behind the gate; its summaries read afterwards"""
    nb, br, _ = VIEW
    L = _L()
    h = C.c_void_p()
    _ck(L.gpemu_diag_create_dev(C.byref(h), 0, _vp(T["chain"]), nb, br * D_WIDE, 0, br, D_WIDE, 0, _vp(st)))
    try:
        res = []
        for kind in (1, 2):                             # RANK_Z, FOLDED_RANK_Z
            gm, mv, vm = (out.host((D_WIDE,)) for _ in range(3))
            _ck(L.gpemu_diag_transform(h, kind, 0.0, _vp(gm), _vp(mv), _vp(vm)))
            res += [gm, mv, vm]
        pooled = [out.host((D_WIDE,)) for _ in range(5)]
        _ck(L.gpemu_diag_pooled(h, *[_vp(a) for a in pooled]))
        return tuple(res + pooled)
    finally:
        L.gpemu_diag_destroy(h)


# ---- model-bound rows: the problems of reuse_cases ------------------------------------------------------------------
def _tag(seed):
    return "" if seed == 0 else f"/decoy{seed}"


def _in_rows(B, tag):
    """B: the number of rows when the inputs are made (a closure over the shape in force)"""
    return lambda P, seed: {"X": R.rows(P, tag + _tag(seed), B())}


def _in_logpost(P, seed):
    """rows all over the box, every seventh outside it (reuse_cases.logpost_rows without the NaN row: a decoy is valid)"""
    X = R.rows(P, "stream_logpost" + _tag(seed), B_BIG)
    X[5::7, 0] = P.hi[0] + 0.25 * (P.hi[0] - P.lo[0])
    return {"X": X}


def _in_model_view(P, seed):
    nb, br, bs = VIEW
    return {"X": R.rows(P, "stream_view" + _tag(seed), nb * bs)}


def _gp_predict(st, T, out, P, dm):
    res = []
    for B in (B_SMALL, B_BIG):
        mean, var = out((B, P.k)), out((B, P.k))
        _ck(_L().gpemu_gp_predict_dev(dm.handle, B, _vp(T["X"]), _vp(mean), _vp(var), _vp(st)))
        res += [mean, var]
    return tuple(res)


def _gp_predict_cov(st, T, out, P, dm):
    M1, M2 = B_SMALL, M2_COV
    mean, cov, sym = out((M1, P.k)), out((P.k, M1, M2)), out((P.k, M1, M1))
    X = T["X"]
    _ck(_L().gpemu_gp_predict_cov_dev(dm.handle, M1, _vp(X), M2, _vp(X[M1:]), 0, _vp(mean), _vp(cov), _vp(st)))
    _ck(_L().gpemu_gp_predict_cov_dev(dm.handle, M1, _vp(X), M1, None, 0, None, _vp(sym), _vp(st)))
    return mean, cov, sym


def _predict_full(st, T, out, P, dm):
    B = B_SMALL
    cv, cov = out((B, P.F)), out((B, P.F, P.F))
    _ck(_L().gpemu_predict_full_dev(dm.handle, B, _vp(T["X"]), 1.0, _vp(cv), _vp(cov), _vp(st)))
    return cv, cov


def _logpost(st, T, out, P, dm):
    res = []
    for B, mode in ((B_SMALL, 0), (B_BIG, 0)) + (() if P.name == "sources" else ((B_SMALL, 1),)):
        o = out((B,))
        _ck(_L().gpemu_logpost_dev(dm.handle, B, _vp(T["X"]), _vp(o), mode, _vp(st)))
        res.append(o)
    return tuple(res)


def _gp_predict_grad(st, T, out, P, dm):
    res = []
    for B in (B_SMALL, B_BIG):
        o = [out((B, P.k)), out((B, P.k)), out((B, P.k, P.d)), out((B, P.k, P.d))]
        _ck(_L().gpemu_gp_predict_grad_dev(dm.handle, B, _vp(T["X"]), *[_vp(a) for a in o], _vp(st)))
        res += o
    return tuple(res)


def _logpost_grad(st, T, out, P, dm):
    res = []
    for B in (B_SMALL, B_BIG):
        lp, g = out((B,)), out((B, P.d))
        _ck(_L().gpemu_logpost_grad_dev(dm.handle, B, _vp(T["X"]), _vp(lp), _vp(g), 0, _vp(st)))
        res += [lp, g]
    return tuple(res)


def _postpred(st, T, out, P, dm):
    nb, br, bs = VIEW
    ranks = i64(0, (nb * br - 1) // 2, nb * br - 1)
    o = [out((P.F,)), out((P.F,)), out((P.F,)), out((P.F, 3))]
    _ck(_L().gpemu_posterior_predictive_dev(dm.handle, _vp(T["X"]), nb, br, bs, 3, _vp(ranks), 0, *[_vp(a) for a in o],
                                            _vp(st)))
    return tuple(o)


def in_weighted_view(P, seed):
    """the rows of a chain view and 2 rows of fixed-point weights, one weight per row of the view"""
    nb, br, bs = VIEW
    q = _fixed_weights(_rng(seed, "wq_view"), RW2, nb * br, 45)          # (16 x 4 rows: in [2^39, 2^40))
    return dict(_in_model_view(P, seed), q=q)


def weighted_bands_run(ctx_of):
    def run(st, T, out, P, dm):
        nb, br, bs = VIEW
        o = [out((RW2, P.F)), out((RW2, P.F)), out((RW2, P.F)), out((RW2, P.F, 3))]
        ctx, ref = _ctx_ref(ctx_of, st)
        _ck(_L().gpemu_posterior_predictive_weighted_dev(dm.handle, _vp(T["X"]), nb, br, bs, RW2, _vp(T["q"]), nb * br, 3,
                                                         _vp(_W_VIEW_TARGETS), *[_vp(a) for a in o], ref))
        return tuple(o)
    return run


def _in_AB(P, seed):
    return {"A": R.rows(P, "stream_A" + _tag(seed), B_SMALL), "B": R.rows(P, "stream_B" + _tag(seed), B_SMALL)}


def _sobol(st, T, out, P, dm):
    return R.flatten(dm.sobol_moments_dev(T["A"].data_ptr(), T["B"].data_ptr(), B_SMALL, n_batches=min(2, B_SMALL),
                                          stream=int(st)))


def _pointwise(st, T, out, P, dm):
    nb, br, bs = VIEW
    o = out((dm.n_observable_blocks, nb * br), ld=nb * br + PAD)
    _ck(_L().gpemu_loglik_pointwise_dev(dm.handle, 0, _vp(T["X"]), nb, br, bs, _vp(o), nb * br + PAD, _vp(st)))
    return (o,)


def _in_design(P, seed):
    nb, br, bs = VIEW
    return {"ref": R.rows(P, "stream_ref" + _tag(seed), nb * bs), "cand": R.rows(P, "stream_cand" + _tag(seed), 70)}


def _design_create(st, T, out, P, dm):
    """the handle created behind the gate; its scores and state read afterwards"""
    nb, br, bs = VIEW
    L = _L()
    h = C.c_void_p()
    pcw = np.ones(P.k)
    _ck(L.gpemu_design_create_dev(C.byref(h), dm.handle, _vp(T["ref"]), nb, br, bs, None, 70, _vp(T["cand"]), _vp(pcw),
                                  None, 1e-6, 4, 0, _vp(st)))
    try:
        s0, s1, iv, den = out.host((70,)), out.host((70,)), out.host((P.k,)), out.host((P.k, 70))
        _ck(L.gpemu_design_scores(h, _vp(s0), None))
        _ck(L.gpemu_design_condition(h, int(np.argmax(s0))))
        _ck(L.gpemu_design_scores(h, _vp(s1), None))
        _ck(L.gpemu_design_state(h, _vp(iv), _vp(den), None))
        return s0, s1, iv, den
    finally:
        L.gpemu_design_destroy(h)


# ---- the sampler ----------------------------------------------------------------------------------------------------
SAMPLER_W = 64


def _in_walkers(P, seed):
    """The start of the ensemble.  It is a HOST input of gpemu_sampler_set_state: the sampler has no device input of
    the caller's, and reading X0 back to the host waits for the gate before the sampler launches anything.  This row
    therefore shows only that the gate was closed when the call began and that a sampler set to a caller's stream runs
    there and gives the quiet device's bits; it cannot catch a launch on the wrong stream.  That check is
    test_sampler_on_a_side_stream_gives_the_same_chain (tests/test_gpu_streams.py)."""
    return {"X0": R.walkers(P, "stream_walkers" + _tag(seed), SAMPLER_W)}


def _sampler_run(st, T, out, P, dm):
    from gpemu.sampler import DeviceSampler
    ds = DeviceSampler([dm], SAMPLER_W, seed=19)
    try:
        _ck(_L().gpemu_sampler_set_stream(ds._h, _vp(st)))
        ds.set_state(T["X0"].cpu().numpy())
        ds.run(3)
        return R.sampler_result(ds)
    finally:
        ds.close()


# ---- the table -------------------------------------------------------------------------------------------------------
ALL4 = ("general", "wide", "tasks10", "sources")
GRAD_CASES = ("general", "tasks10")      # the derivatives decline Matern 0.75 ("wide") and correlated sources
_M_NOWAIT = dict(family=MODEL_BOUND, null_means=NULL_MODEL, waits=False,
                 doc=(("NULL = the model's own stream", "conventions"), (NOWAIT, "conventions")))
_M_WAIT = dict(family=MODEL_BOUND, null_means=NULL_MODEL, waits=True,
               doc=(("(NULL = the model's) and waits for it", "section"),))
_WIDE = dict(family=DEVICE_WIDE, null_means=NULL_NULL, waits=True, doc=((NULL_NULL, "section"), (WAITS, "section")))
# the entries whose stream is ctx->stream: their section names them one by one
_CTX_WIDE = dict(family=DEVICE_WIDE, null_means=NULL_NULL, waits=True,
                 doc=(("work on ctx->stream (NULL = the null stream) and each waits for it before returning", "section"),))
_CTX_MODEL = dict(family=MODEL_BOUND, null_means=NULL_MODEL, waits=True,
                  doc=(("works on ctx->stream (NULL = the model's) and waits for it before returning", "section"),))

# edge_shapes: the guard sweep's shapes of a row, from the sets above (where each set's tile, chunk and wave sizes are
# cited by file and constant); out_ld, gaps: what tests/guard_cases.py pads and fills
ROWS = [
    Row("gpemu_gp_predict_dev", inputs=_in_rows(lambda: B_BIG, "stream_gp"), run=_gp_predict, cases=ALL4, edge_shapes=B_EDGES, **_M_NOWAIT),
    Row("gpemu_gp_predict_cov_dev", inputs=_in_rows(lambda: B_SMALL + M2_COV, "stream_pcov"), run=_gp_predict_cov, cases=ALL4,
        edge_shapes=PCOV_EDGES,
        **_M_WAIT),                      # (its workspace goes with the call)
    Row("gpemu_predict_full_dev", inputs=_in_rows(lambda: B_SMALL, "stream_full"), run=_predict_full, cases=ALL4,
        # k_exact.hip launch_predict_full: the matrix-core writer stores pairs (16 bytes) and runs where dcov is 16-byte
        # aligned and F even; the row-wise writer otherwise (other bits: include/gpemu.h).  PM_NB samples per group.
        by_alignment=True, edge_shapes=B_EDGES + tuple(dataclasses.replace(sh, a16=True) for sh in B_EDGES), **_M_NOWAIT),
    Row("gpemu_logpost_dev", inputs=_in_logpost, run=_logpost, cases=ALL4, edge_shapes=B_EDGES, **_M_NOWAIT),
    Row("gpemu_gp_predict_grad_dev", inputs=_in_rows(lambda: B_BIG, "stream_pgrad"), run=_gp_predict_grad, cases=GRAD_CASES,
        edge_shapes=B_EDGES, **_M_NOWAIT),
    Row("gpemu_logpost_grad_dev", inputs=_in_logpost, run=_logpost_grad, cases=GRAD_CASES, edge_shapes=B_EDGES, **_M_NOWAIT),
    Row("gpemu_sampler_set_stream", family=SAMPLER_COMM, null_means=NULL_FIRST_GROUP, waits=True,
        doc=((NULL_FIRST_GROUP, "section"), ("gpemu_sampler_run waits for it", "section")),
        inputs=_in_walkers, run=_sampler_run, cases=("general",), edge_shapes=(Shape(),)),   # (W is the sampler's own)
    Row("gpemu_comm_all_gather", family=SAMPLER_COMM, null_means=NULL_NULL, waits=False,
        doc=(("enqueued on `stream` (NULL = the null stream); does not wait", "section"),),
        omitted="needs RCCL and more than one rank: tests/test_gpu_dropin.py runs it under torch.distributed"),
    Row("gpemu_select_dev", inputs=_in_V, run=_select, edge_shapes=WIDE_V + S_CHUNK_2048 + S_CHUNK_4096, **_WIDE),
    Row("gpemu_posterior_predictive_dev", inputs=_in_model_view, run=_postpred, cases=ALL4, gaps=("X",), edge_shapes=VIEW_EDGES,
        **_M_WAIT),
    Row("gpemu_rank_dev", inputs=_in_V, run=_rank, edge_shapes=WIDE_V + S_CHUNK_2048, **_WIDE),
    Row("gpemu_diag_create_dev", inputs=_in_chain, run=_diag_create, edge_shapes=VIEW_EDGES + (Shape(VIEW=(17, 4, 9), D=1),
                                                                                               Shape(VIEW=(17, 4, 9), D=16)),
        **dict(_WIDE, family=HANDLE_CREATING)),
    Row("gpemu_sobol_moments_dev", inputs=_in_AB, run=_sobol, cases=ALL4, edge_shapes=B_EDGES,
        **_M_WAIT),
    Row("gpemu_marginal_hist_dev", inputs=_in_X, run=_hist, edge_shapes=WIDE_S, **_WIDE),
    Row("gpemu_hpd_dev", inputs=_in_V, run=_hpd, edge_shapes=WIDE_V + S_CHUNK_2048 + S_CHUNK_4096, **_WIDE),
    Row("gpemu_kde1d_dev", inputs=_in_V, run=_kde1d, edge_shapes=WIDE_V + S_CHUNK_1024 + S_CHUNK_8192, **_WIDE),
    Row("gpemu_marginal_dense_dev", inputs=_in_view, run=_dense, gaps=("X",),
        edge_shapes=VIEW_EDGES + (Shape(VIEW=(17, 4, 9), D=1), Shape(VIEW=(17, 4, 9), D=16)), **_WIDE),
    Row("gpemu_marginal_moments_dev", inputs=_in_X, run=_moments, edge_shapes=WIDE_S + S_CHUNK_1024, **_WIDE),
    Row("gpemu_kde2d_dev", inputs=_in_X, run=_kde2d, edge_shapes=WIDE_S + S_CHUNK_8192, **_WIDE),
    Row("gpemu_pair_moments_dev", inputs=_in_X, run=_pair_moments, edge_shapes=WIDE_S + S_CHUNK_1024, **_WIDE),
    Row("gpemu_loglik_pointwise_dev", inputs=_in_model_view, run=_pointwise, cases=("general", "wide", "tasks10"),
        gaps=("X",), out_ld=("ldt",), edge_shapes=VIEW_EDGES,
        **_M_WAIT),                      # (the per-observable terms decline correlated sources)
    Row("gpemu_psis_dev", inputs=_in_loglik_rows, run=_psis, edge_shapes=WIDE_V + S_CHUNK_2048 + S_CHUNK_4096, **_WIDE),
    Row("gpemu_weighted_moments_dev", inputs=_in_X_logw, run=_weighted_moments, edge_shapes=WIDE_S + S_CHUNK_4096,
        **_WIDE),
    Row("gpemu_loo_group_rows_dev", inputs=_in_loglik_rows, run=_group_rows, out_ld=("ldo",), edge_shapes=WIDE_V,
        **_WIDE),
    Row("gpemu_design_create_dev", family=HANDLE_CREATING, null_means=NULL_NONE, waits=True,
        doc=(("`stream` (NULL: none) is waited for before the rows are read", "section"),
             ("every call waits for it", "section")),
        inputs=_in_design, run=_design_create, cases=ALL4, gaps=("ref",), edge_shapes=VIEW_EDGES),
    Row("gpemu_unit_rows_dev", inputs=_in_X, run=_unit, edge_shapes=WIDE_S, **_WIDE),
    Row("gpemu_knn_dist_dev", inputs=_in_X, run=_knn_dist, edge_shapes=WIDE_S, **_WIDE),
    Row("gpemu_knn_logsum_dev", inputs=_in_r2, run=_knn_logsum, edge_shapes=WIDE_V + S_CHUNK_1024, **_WIDE),
    Row("gpemu_pair_lse_dev", inputs=_in_YZ, run=_pair_lse, edge_shapes=WIDE_V + S_CHUNK_2048 + B_EDGES[:8], **_WIDE),
    Row("gpemu_pairlse_centre_dev", inputs=_in_YZ, run=_centre, edge_shapes=WIDE_V + S_CHUNK_1024, **_WIDE),
    Row("gpemu_logprior_dev", inputs=_in_X, run=_logprior, out_ld=("ldl",), edge_shapes=WIDE_S, **_WIDE),
    Row("gpemu_logmeanexp_dev", inputs=_in_L, run=_logmeanexp, edge_shapes=WIDE_V + S_CHUNK_4096, **_WIDE),
    Row("gpemu_weights_fixed_dev", inputs=_in_lw, run=_weights_fixed, out_ld=("ldq",), edge_shapes=WIDE_V, **_WIDE),
    Row("gpemu_weighted_select_dev", inputs=_in_Vq, run=_weighted_select, edge_shapes=WIDE_S + S_CHUNK_2048 + S_CHUNK_4096,
        **_WIDE),
    Row("gpemu_weighted_hist_dev", inputs=_in_Vq, run=_weighted_hist, edge_shapes=WIDE_S, **_WIDE),
    Row("gpemu_posterior_predictive_weighted_dev", inputs=in_weighted_view, run=weighted_bands_run(ctx_on),
        cases=("general", "wide"), gaps=("X",), edge_shapes=VIEW_EDGES, **_CTX_MODEL),
    Row("gpemu_weighted_hpd_dev", inputs=_in_Vq2, run=weighted_hpd_run(ctx_on), edge_shapes=WIDE_V + S_CHUNK_2048 + S_CHUNK_4096,
        **_CTX_WIDE),
    Row("gpemu_weighted_kde1d_dev", inputs=_in_Vq2, run=weighted_kde_run(ctx_on), edge_shapes=WIDE_V + S_CHUNK_8192,
        **_CTX_WIDE),
]
ROW = {r.name: r for r in ROWS}


# the ld* / stride parameters of the prototypes that address an INPUT (every other one belongs to an output and is named
# in its row's ``out_ld``: tests/test_guards_host.py)
INPUT_LD = {
    "gpemu_select_dev": ("row_stride", "elem_stride"), "gpemu_rank_dev": ("row_stride", "elem_stride"),
    "gpemu_hpd_dev": ("row_stride", "elem_stride"), "gpemu_kde1d_dev": ("row_stride", "elem_stride"),
    "gpemu_psis_dev": ("row_stride", "elem_stride"), "gpemu_diag_create_dev": ("step_stride",),
    "gpemu_posterior_predictive_dev": ("block_stride_rows",), "gpemu_marginal_hist_dev": ("block_stride_rows",),
    "gpemu_marginal_dense_dev": ("block_stride_rows",), "gpemu_kde2d_dev": ("block_stride_rows",),
    "gpemu_pair_moments_dev": ("block_stride_rows",), "gpemu_loglik_pointwise_dev": ("block_stride_rows",),
    "gpemu_weighted_moments_dev": ("block_stride_rows", "ldw"), "gpemu_loo_group_rows_dev": ("ldt",),
    "gpemu_design_create_dev": ("block_stride_rows",), "gpemu_unit_rows_dev": ("block_stride",),
    "gpemu_pair_lse_dev": ("ldy", "ldz"), "gpemu_pairlse_centre_dev": ("ldz",),
    "gpemu_logprior_dev": ("block_stride_rows",), "gpemu_logmeanexp_dev": ("ldl",), "gpemu_weights_fixed_dev": ("ldw",),
    "gpemu_weighted_select_dev": ("row_stride", "elem_stride", "ldq"),
    "gpemu_weighted_hist_dev": ("block_stride_rows", "ldq"),
    "gpemu_posterior_predictive_weighted_dev": ("block_stride_rows", "ldq"),
    "gpemu_weighted_hpd_dev": ("row_stride", "elem_stride", "ldq"),
    "gpemu_weighted_kde1d_dev": ("row_stride", "elem_stride", "ldq"),
}


@contextmanager
def shaped(sh):
    """the module's shape constants, and the tables made from them, rebound to ``sh`` while the block runs"""
    g = globals()
    tables = _w_tables(sh.RW)
    new = dict(S_WIDE=sh.S, D_WIDE=sh.D, VIEW=tuple(sh.VIEW), B_SMALL=sh.B_SMALL, B_BIG=sh.B_BIG, RW2=sh.RW, M2_COV=sh.M2,
               PAD=sh.pad, A16=sh.a16, EDGES1=_edges(8, sh.D), EDGES2=_edges(4, sh.D), _W_TARGETS=tables[0], _W_GRID=tables[1],
               _W_H=tables[2], _W_VIEW_TARGETS=tables[3])
    old = {k: g[k] for k in new}
    g.update(new)
    try:
        yield sh
    finally:
        g.update(old)


def gap_mask(shape):
    """of the rows of a view's input [nb*bs][d]: True where a row lies between the blocks (VIEW in force)"""
    nb, br, bs = VIEW
    m = np.zeros(shape, dtype=bool)
    m.reshape(nb, bs, -1)[:, br:] = True
    return m


def sweep_params(families):
    """(row, case) of every row of these families that the GPU sweep runs; case None for a row without a model"""
    return [(r, c) for r in ROWS if r.family in families and not r.omitted for c in (r.cases or (None,))]


def param_id(rc):
    return rc[0].name.replace("gpemu_", "") + ("" if rc[1] is None else f"-{rc[1]}")


# ---- the gate --------------------------------------------------------------------------------------------------------
_CYCLES_PER_MS = None
LATENCIES = {}                            # row -> longest host time [ms] from the gate's enqueue, see the docstring


def calibrate():
    """cycles of ``torch.cuda._sleep`` per millisecond on this device, timed once with torch events"""
    global _CYCLES_PER_MS
    if _CYCLES_PER_MS is None:
        import torch
        torch.cuda.synchronize()
        n = 20_000_000
        torch.cuda._sleep(1000)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(n)
        e1.record()
        e1.synchronize()
        _CYCLES_PER_MS = n / e0.elapsed_time(e1)
        print(f"[streams] gate calibration: {1e6 / _CYCLES_PER_MS:.4f} ms per 1e6 cycles of _sleep; gate {GATE_MS} ms")
    return _CYCLES_PER_MS


def _device(T):
    import torch
    dev = torch.device("cuda", 0)
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in T.items()}


class Outs:
    """the allocator of a closure's device outputs: fresh tensors of NaN (integers: -1), or the ones made before"""

    def __init__(self, pre=None, odd=False):
        """``odd``: the tensors start 8 bytes past a 16-byte boundary (torch's own are aligned to 512 bytes)"""
        self.made, self.pre, self.odd = [], pre, odd

    def __call__(self, shape, dtype=None, ld=None):
        """``ld``: the leading dimension of a matrix, at least its row length; the rows of the result lie ld apart"""
        import torch
        dtype = dtype or torch.float64
        if self.pre is not None:
            t = self.pre[len(self.made)]
            assert tuple(t.shape) == tuple(shape) and t.dtype == dtype
        elif self.odd:
            assert ld is None or ld == shape[-1]
            t = blank((int(np.prod(shape)) + 1,), dtype)[1:].view(tuple(shape))
        elif ld is None or ld == shape[-1]:
            t = blank(shape, dtype)
        else:
            assert len(shape) == 2 and ld > shape[1]
            t = blank((shape[0], ld), dtype)[:, :shape[1]]
        self.made.append(t)
        return t

    def host(self, shape, dtype=np.float64):
        """a host output: NaN (integers: -1)"""
        return np.full(shape, np.nan if np.dtype(dtype).kind == "f" else -1, dtype=dtype)


def blank(shape, dtype):
    import torch
    return torch.full(tuple(shape), float("nan") if dtype.is_floating_point else -1, dtype=dtype,
                      device=torch.device("cuda", 0))


def _host(res):
    import torch
    return tuple(np.array(r.cpu().numpy() if torch.is_tensor(r) else r, copy=True) for r in res)


def quiet(row, P, dm, inputs, st=0, odd=False):
    """the call on a quiet device with the default stream argument: (results, the outputs it allocated)"""
    import torch
    T = _device(inputs)
    o = Outs(odd=odd)
    torch.cuda.synchronize()
    res = row.run(st, T, o, P, dm)
    torch.cuda.synchronize()
    return _host(res), o.made


def gated(row, P, dm, true, decoy, s, like, null=False):
    """the call behind a closed gate on the torch stream ``s`` (``null``: NULL is passed, ``s`` is torch's default
    stream); ``like``: the outputs of a quiet run, for the shapes.  Returns the results as host arrays."""
    import torch
    cycles = int(calibrate() * GATE_MS)
    T, src = _device(decoy), _device(true)
    o = Outs([blank(t.shape, t.dtype) for t in like])
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        t0 = time.perf_counter()
        torch.cuda._sleep(cycles)
        for k in T:
            T[k].copy_(src[k], non_blocking=True)
        closed_before = not s.query()
        t1 = time.perf_counter()
        res = row.run(0 if null else s.cuda_stream, T, o, P, dm)
        t2 = time.perf_counter()
        closed_after = not s.query()
        res = tuple(r.clone() if torch.is_tensor(r) else r for r in res)
        s.synchronize()
    ms = 1e3 * ((t1 if row.waits else t2) - t0)
    LATENCIES[row.name] = max(LATENCIES.get(row.name, 0.0), ms)
    print(f"[streams] {row.name}: {ms:.3f} ms of host time behind the gate")
    assert closed_before, (f"{row.name}: the gate of {GATE_MS} ms had opened before the call was made "
                           f"({1e3 * (t1 - t0):.2f} ms after its enqueue): the run proves nothing")
    if not row.waits:
        assert closed_after, (f"{row.name} is documented not to wait, but the stream had run empty when it returned "
                              f"({1e3 * (t2 - t0):.2f} ms after the gate's enqueue, gate {GATE_MS} ms): it waited for the "
                              f"stream, or the gate is too short")
    return _host(res)


def differs(a, b):
    return len(a) != len(b) or any(not R.same_bits(x, y) for x, y in zip(a, b))


def assert_same(what, got, want):
    assert len(got) == len(want) and len(want) > 0, f"{what}: {len(got)} arrays, {len(want)} on the quiet device"
    for i, (a, b) in enumerate(zip(got, want)):
        if not R.same_bits(a, b):
            bad = np.flatnonzero(~((a == b) | ((a != a) & (b != b))).reshape(-1)) if a.shape == b.shape else []
            raise AssertionError(f"{what}: array {i} of shape {a.shape} differs from the quiet device's in {len(bad)} "
                                 f"elements, first at {bad[:5]}: got {a.reshape(-1)[bad[:3]]}, want {b.reshape(-1)[bad[:3]]}")
