"""Positions and training rows up to the eight symmetries of the square (csrc/canon.hip).

    c_own, c_opp, sym, stab = canon(own, opp)            # the canonical image of each position
    pi_c, act_c = transform_rows(pi, act, sym, stab)     # the rows' payload in that frame
    pi_s = symmetrise(pi_c, stab)                        # averaged over the stabiliser

sym = k + 4 * flip is oth_d4's numbering (rot90 k times, then fliplr).  The canonical image
is the smallest (d4(own, s), d4(opp, s)) as unsigned words, own first; `sym` the smallest s
that attains it; bit t of `stab` says that symmetry t fixes the canonical pair.  A position
with overlapping boards is passed through with sym = AZ_CANON_BAD (255) and stab = 0, and
its rows come out as NaN / 255.

NumPy in gives NumPy out -- computed on the host (oth_canon_cpu and friends over at most 16
threads) unless `device` names a GPU; CUDA tensors in give CUDA tensors out, asynchronously
on the current stream.  Boards are uint64 arrays on the host and int64 tensors holding the
same bits on the device, as everywhere else.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

import az_native as nat
from endgame import MAX_THREADS

BAD = nat.AZ_CANON_BAD


def _slices(n, grain):
    """Bounds of at most MAX_THREADS slices of n items, none smaller than `grain`."""
    k = max(1, min(MAX_THREADS, n // grain))
    return np.linspace(0, n, k + 1).astype(np.int64)


def _pool(run, bounds):
    """run(a, b) for every slice; the ctypes calls release the GIL."""
    pairs = [(int(bounds[i]), int(bounds[i + 1])) for i in range(len(bounds) - 1)]
    if len(pairs) == 1:
        run(*pairs[0])
        return
    with ThreadPoolExecutor(len(pairs)) as ex:
        list(ex.map(lambda ab: run(*ab), pairs))


def _cut(x, a, b):
    return None if x is None else x[a:b]


def _to_np(x, dt):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if dt == np.uint64 and x.dtype == np.int64:
        x = x.view(np.uint64)
    return np.ascontiguousarray(x, dtype=dt)


def _to_dev(x, dt, dev):
    if x is None:
        return None
    if not isinstance(x, torch.Tensor):
        x = np.ascontiguousarray(x)
        x = torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x)
    return x.to(device=dev, dtype=dt).contiguous()


def _side(device, *xs):
    """(device to compute on, whether the caller gets torch tensors back)."""
    first = next(x for x in xs if x is not None)
    want_torch = isinstance(first, torch.Tensor)
    if device is not None:
        return torch.device(device), want_torch
    return (first.device if want_torch else torch.device("cpu")), want_torch


# ---- the entry points on one side ------------------------------------------------------

def canon_cpu(own, opp):
    """oth_canon_cpu on uint64 arrays: (own, opp, sym uint8, stab uint8)."""
    own, opp = _to_np(own, np.uint64).reshape(-1), _to_np(opp, np.uint64).reshape(-1)
    n = own.size
    o, p = np.empty(n, np.uint64), np.empty(n, np.uint64)
    sym, stab = np.empty(n, np.uint8), np.empty(n, np.uint8)

    def run(a, b):
        nat.check(nat.lib.oth_canon_cpu(nat.ptr(own[a:b]), nat.ptr(opp[a:b]), b - a,
                                        nat.ptr(o[a:b]), nat.ptr(p[a:b]), nat.ptr(sym[a:b]),
                                        nat.ptr(stab[a:b])), "oth_canon_cpu")

    _pool(run, _slices(n, 4096))
    return o, p, sym, stab


def canon_gpu(own, opp, stream=None):
    """oth_canon_gpu on int64 device tensors (contiguous, any alignment): device tensors
    (own, opp, sym uint8, stab uint8), asynchronous on `stream`."""
    dev = own.device
    n = int(own.numel())
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            o, p = torch.empty_like(own), torch.empty_like(opp)
            sym = torch.empty(n, dtype=torch.uint8, device=dev)
            stab = torch.empty(n, dtype=torch.uint8, device=dev)
            nat.check(nat.lib.oth_canon_gpu(nat.ptr(own), nat.ptr(opp), n, nat.ptr(o), nat.ptr(p),
                                            nat.ptr(sym), nat.ptr(stab), nat.stream_ptr(s)),
                      "oth_canon_gpu")
    return o, p, sym, stab


def rows_d4_cpu(pi, act, sym, stab):
    """az_rows_d4_cpu: (pi_o float32 [n, 65], act_o uint8 [n]); pi, act and stab may be None."""
    pi, act = _to_np(pi, np.float32), _to_np(act, np.uint8)
    sym, stab = _to_np(sym, np.uint8).reshape(-1), _to_np(stab, np.uint8)
    n = sym.size
    pi = None if pi is None else pi.reshape(n, 65)
    pi_o = None if pi is None else np.empty((n, 65), np.float32)
    act_o = None if act is None else np.empty(n, np.uint8)

    def run(a, b):
        nat.check(nat.lib.az_rows_d4_cpu(nat.ptr(_cut(pi, a, b)), nat.ptr(_cut(act, a, b)),
                                         nat.ptr(sym[a:b]), nat.ptr(_cut(stab, a, b)), b - a,
                                         nat.ptr(_cut(pi_o, a, b)), nat.ptr(_cut(act_o, a, b))),
                  "az_rows_d4_cpu")

    _pool(run, _slices(n, 1024))
    return pi_o, act_o


def rows_d4_gpu(pi, act, sym, stab, stream=None):
    """az_rows_d4_gpu on contiguous device tensors, asynchronous on `stream`."""
    dev = sym.device
    n = int(sym.numel())
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            pi_o = None if pi is None else torch.empty((n, 65), dtype=torch.float32, device=dev)
            act_o = None if act is None else torch.empty(n, dtype=torch.uint8, device=dev)
            nat.check(nat.lib.az_rows_d4_gpu(nat.ptr(pi), nat.ptr(act), nat.ptr(sym),
                                             nat.ptr(stab), n, nat.ptr(pi_o), nat.ptr(act_o),
                                             nat.stream_ptr(s)), "az_rows_d4_gpu")
    return pi_o, act_o


def symmetrise_cpu(pi, stab):
    """az_rows_symmetrise_cpu: float32 [n, 65]."""
    stab = _to_np(stab, np.uint8).reshape(-1)
    n = stab.size
    pi = _to_np(pi, np.float32).reshape(n, 65)
    out = np.empty((n, 65), np.float32)

    def run(a, b):
        nat.check(nat.lib.az_rows_symmetrise_cpu(nat.ptr(pi[a:b]), nat.ptr(stab[a:b]), b - a,
                                                 nat.ptr(out[a:b])), "az_rows_symmetrise_cpu")

    _pool(run, _slices(n, 1024))
    return out


def symmetrise_gpu(pi, stab, stream=None):
    """az_rows_symmetrise_gpu on contiguous device tensors, asynchronous on `stream`."""
    dev = stab.device
    n = int(stab.numel())
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            out = torch.empty((n, 65), dtype=torch.float32, device=dev)
            nat.check(nat.lib.az_rows_symmetrise_gpu(nat.ptr(pi), nat.ptr(stab), n, nat.ptr(out),
                                                     nat.stream_ptr(s)), "az_rows_symmetrise_gpu")
    return out


# ---- public interface ------------------------------------------------------------------

def _back(res, want_torch, like):
    """Results of one side -> what the caller asked for (None entries stay None)."""
    out = []
    for r in res:
        if r is None:
            out.append(None)
        elif want_torch:
            if not isinstance(r, torch.Tensor):
                r = torch.from_numpy(r.view(np.int64) if r.dtype == np.uint64 else r)
            out.append(r.to(like.device))
        else:
            if isinstance(r, torch.Tensor):
                r = r.cpu().numpy()
            out.append(r.view(np.uint64) if r.dtype == np.int64 else r)
    return tuple(out)


def canon(own, opp, device=None):
    """(own, opp, sym, stab) of every position's canonical image, shaped [n]."""
    dev, want_torch = _side(device, own)
    if dev.type == "cuda":
        res = canon_gpu(_to_dev(own, torch.int64, dev).reshape(-1),
                        _to_dev(opp, torch.int64, dev).reshape(-1))
    else:
        res = canon_cpu(own, opp)
    return _back(res, want_torch, own)


def transform_rows(pi=None, act=None, sym=None, stab=None, device=None):
    """Apply each row's `sym` to its payload: (pi_o, act_o), None where the input was None.
    pi [n, 65] float32: pi_o[d4_square(j, sym)] = pi[j], the pass entry stays.  act [n] uint8:
    d4_square(act, sym), then with `stab` the smallest square of its orbit under stab; the
    pass (64) stays."""
    if sym is None or (pi is None and act is None):
        raise ValueError("transform_rows needs sym and at least one of pi, act")
    dev, want_torch = _side(device, pi, act)
    if dev.type == "cuda":
        res = rows_d4_gpu(_to_dev(pi, torch.float32, dev), _to_dev(act, torch.uint8, dev),
                          _to_dev(sym, torch.uint8, dev).reshape(-1),
                          _to_dev(stab, torch.uint8, dev))
    else:
        res = rows_d4_cpu(pi, act, sym, stab)
    return _back(res, want_torch, pi if pi is not None else act)


def symmetrise(pi, stab, device=None):
    """Average pi [n, 65] over each row's stabiliser: exactly equal entries on the squares of
    an orbit (see include/az_othello.h for the summation order); rows with stab == 1 are
    copied."""
    dev, want_torch = _side(device, pi)
    if dev.type == "cuda":
        res = symmetrise_gpu(_to_dev(pi, torch.float32, dev),
                             _to_dev(stab, torch.uint8, dev).reshape(-1))
    else:
        res = symmetrise_cpu(pi, stab)
    return _back((res,), want_torch, pi)[0]
