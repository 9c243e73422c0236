"""Array-level API over libctg.so: RAG + edge features of a label volume.

Inputs are numpy arrays (host memory, results come back as numpy) or torch
CUDA tensors (device memory, results stay resident as torch tensors).  This is
the layer that ``cluster_tools_amd.ndist`` (the ``nifty.distributed`` mirror)
calls after reading blocks from N5.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import sys
import threading

import numpy as np

from . import _lib as L

N_FEATURES = L.CTG_N_FEATURES
NBINS = L.CTG_NBINS
WIDE_WORDS = L.CTG_WIDE_RECORD_WORDS
NSLOTS = NBINS + 2   # histogram slots of a wide record: left outliers, the bins, right outliers
MORPH_COLS = L.CTG_MORPH_COLS   # [id, size, com z y x, min z y x, max z y x]
MORPH_WORDS = 10               # [n, sum z y x, min z y x, max z y x]
REGION_COLS = L.CTG_REGION_COLS   # [id, count, sum, min, max] or [id, count, mean, minimum, maximum]
REGION_FEATURE_NAMES = ('count', 'mean', 'minimum', 'maximum')   # the feature form's columns after the id


def _region_form(form):
    try:
        return {'sums': L.CTG_REGION_SUMS, 'features': L.CTG_REGION_FEATURES}[form]
    except KeyError:
        raise ValueError("form must be 'sums' or 'features', got %r" % (form,)) from None


def _is_torch(x):
    """x is a torch tensor -- without importing torch: a process that never
    imported it holds no tensors (a drop-in job process would otherwise pay
    torch's ~1.4 s import on its first library call)."""
    torch = sys.modules.get('torch')
    return torch is not None and isinstance(x, torch.Tensor)


def _ptr(x):
    if x is None:
        return None
    if _is_torch(x):
        return ctypes.c_void_p(x.data_ptr())
    return x.ctypes.data_as(ctypes.c_void_p)


def _shape_arr(vals):
    """Three int64 for the library; None stays a null pointer (the library's default)."""
    return None if vals is None else (ctypes.c_int64 * 3)(*[int(v) for v in vals])


def _handle_stream(stream=None):
    """The stream of a call that reads a device-resident handle: ``stream``,
    else torch's current stream where torch runs on the GPU in this process
    (the handle's call took the same), else the null stream."""
    if stream is not None:
        return stream
    torch = sys.modules.get('torch')
    if torch is None or not torch.cuda.is_initialized():
        return None
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _stream(stream, on_dev):
    """The stream of a call: ``stream``, else torch's current one for tensor inputs, else the null stream."""
    if stream is not None or not on_dev:
        return stream
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _mem(on_dev):
    return L.CTG_MEM_DEVICE if on_dev else L.CTG_MEM_HOST


class _Handle:
    """Owning wrapper around a handle of the library (device-resident): freed
    by free(), at the end of a ``with`` block, or at the latest with the object."""
    _free = None   # the name of the library's free function

    def __init__(self, handle, device):
        self.handle = handle
        self.device = device

    def free(self):
        if getattr(self, 'handle', None) and L is not None:
            getattr(L.load(), self._free)(self.handle)
            self.handle = None

    __del__ = free

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def _create(cls, fn, *args):
    """lib.<fn>(*args, &handle) on the current device, checked -> cls(handle, device)."""
    lib = L.load()
    dev = L.init_device()
    h = ctypes.c_void_p()
    L.check(getattr(lib, fn)(*args, ctypes.byref(h)), fn)
    return cls(h, dev)


class Result(_Handle):
    """Owning wrapper around a ``ctg_result*`` handle (device-resident)."""
    _free = 'ctg_free'
    # ctg_result_copy_<name>: the attribute with the number of rows, and per output the rest of its shape and its dtype
    _TABLES = {
        'edges': ('n_edges', [((2,), np.uint64)]),
        'nodes': ('n_nodes', [((), np.uint64)]),
        'features': ('n_edges', [((N_FEATURES,), np.float64)]),
        'stats': ('n_edges', [((2,), np.float64), ((WIDE_WORDS,), np.uint32)]),
        'counts': ('n_edges', [((), np.uint64)]),
        'moments': ('n_nodes', [((MORPH_WORDS,), np.uint64)]),
        'region': ('n_nodes', [((), np.uint64), ((), np.float64), ((2,), np.float32)]),
    }

    @property
    def n_edges(self):
        return int(L.load().ctg_result_num_edges(self.handle))

    @property
    def n_nodes(self):
        return int(L.load().ctg_result_num_nodes(self.handle))

    def info(self):
        a, b = ctypes.c_int64(), ctypes.c_int64()
        L.check(L.load().ctg_result_info(self.handle, ctypes.byref(a), ctypes.byref(b)), 'ctg_result_info')
        return int(a.value), int(b.value)

    def _new(self, n, tail, dtype, on_dev):
        """A new output of ``n`` rows: a numpy array, or with ``on_dev`` a tensor on the handle's device
        (unsigned words as the signed type of their width)."""
        if not on_dev:
            return np.empty((n,) + tail, dtype=dtype)
        import torch
        return torch.empty((n,) + tail, dtype=getattr(torch, dtype.__name__.replace('uint', 'int')),
                           device='cuda:%d' % self.device)

    def _copy(self, name, on_dev=False):
        """The table(s) ``name`` of _TABLES in new host arrays, or with ``on_dev`` in new tensors."""
        count, specs = self._TABLES[name]
        n = getattr(self, count)
        outs = [self._new(n, tail, dtype, on_dev) for tail, dtype in specs]
        if on_dev:
            self._before_device_copy()
        rc = getattr(L.load(), 'ctg_result_copy_' + name)(self.handle, *[_ptr(o) for o in outs], _mem(on_dev))
        L.check(rc, 'device copy' if on_dev and len(outs) == 1 else 'copy_' + name)
        return outs[0] if len(outs) == 1 else tuple(outs)

    def _rows(self, fn, cols, args, on_dev, stream):
        """The float64 rows of every node, ids ascending: lib.<fn>(handle, 0, 0, *args, no dense table, rows, ...)."""
        out = self._new(self.n_nodes, (cols,), np.float64, on_dev)
        L.check(getattr(L.load(), fn)(self.handle, 0, 0, *args, None, _ptr(out), _mem(on_dev),
                                      _handle_stream(stream)), fn)
        return out

    @staticmethod
    def _before_device_copy():
        """The accessors copy on a stream of the library's own, ordered after
        nothing else: a fresh tensor may be a block of torch's allocator that
        work queued on the current stream still uses, so that work ends first."""
        import torch
        torch.cuda.current_stream().synchronize()

    # --- host copies
    def edges(self):
        return self._copy('edges')

    def nodes(self):
        return self._copy('nodes')

    def features(self):
        return self._copy('features')

    def stats(self):
        """(sums (E,2) float64, records (E,48) uint32) wide statistics."""
        return self._copy('stats')

    def counts(self):
        """(E,) uint64 voxel counts of an overlaps result."""
        return self._copy('counts')

    def moments(self):
        """(N,10) uint64 moments of a morphology result."""
        return self._copy('moments')

    def morph_rows(self, stream=None):
        """(N,11) float64 rows of a morphology result, ids ascending."""
        return self._rows('ctg_morphology_rows', MORPH_COLS, (), False, stream)

    def region_moments(self):
        """(counts (N,) uint64, sums (N,) float64, minmax (N,2) float32) of a
        region-features result."""
        return self._copy('region')

    def region_rows(self, form='sums', norm=1.0, stream=None):
        """(N,5) float64 rows of a region-features result, ids ascending:
        [id, count, sum, min, max] (``form`` 'sums') or [id, count, mean,
        minimum, maximum] over ``norm`` ('features')."""
        return self._rows('ctg_region_rows', REGION_COLS, (_region_form(form), float(norm)), False, stream)

    # --- device copies (torch); uint64 tables as int64 tensors, the records as int32
    def region_rows_torch(self, form='sums', norm=1.0, stream=None):
        """(N,5) float64 tensor of the rows of a region-features result."""
        return self._rows('ctg_region_rows', REGION_COLS, (_region_form(form), float(norm)), True, stream)

    def moments_torch(self):
        """(N,10) int64 tensor of the uint64 moments of a morphology result."""
        return self._copy('moments', True)

    def morph_rows_torch(self, stream=None):
        """(N,11) float64 tensor of the rows of a morphology result."""
        return self._rows('ctg_morphology_rows', MORPH_COLS, (), True, stream)

    def counts_torch(self):
        """(E,) int64 tensor of the uint64 counts of an overlaps result."""
        return self._copy('counts', True)

    def edges_torch(self):
        import torch
        t = self._copy('edges', True)
        return t.view(torch.uint64) if hasattr(torch, 'uint64') else t

    def nodes_torch(self):
        return self._copy('nodes', True)

    def edges_torch_i64(self):
        """(E,2) int64 view of the uint64 edge table (labels < 2^63)."""
        return self._copy('edges', True)

    def features_torch(self):
        return self._copy('features', True)

    def stats_torch(self):
        return self._copy('stats', True)


def _box(shape, begin, end):
    """The box [begin, end) of a dense-volume call on an array of ``shape`` -> (b, e, oshape)."""
    for box in (begin, end):
        if box is not None and len(box) != 3:
            raise ValueError('begin / end must have 3 entries')
    b = [0, 0, 0] if begin is None else [int(v) for v in begin]
    e = list(shape) if end is None else [int(v) for v in end]
    if any(not 0 <= lo <= hi <= sh for lo, hi, sh in zip(b, e, shape)):
        raise ValueError('box [%s, %s) outside the array of shape %s' % (b, e, shape))
    return b, e, tuple(hi - lo for lo, hi in zip(b, e))


def _dense_out(out, oshape, on_dev, like, kind, name, what=None):
    """The output of a dense call: a new array of ``oshape`` of the kind of ``like`` (numpy, or a tensor on
    its device), or ``out`` checked against it.  ``kind``: 'int64' (uint64 arrays, int64 tensors; either
    64-bit integer type passes), 'float32' or 'float64'; ``name``: what the messages call ``like``;
    ``oshape``: a shape, or an int where only the size counts; ``what``: that shape in the last message
    (default: the shape of the box)."""
    if out is None:
        if on_dev:
            import torch
            return torch.empty(oshape, dtype=getattr(torch, kind), device=like.device)
        return np.empty(oshape, dtype=np.uint64 if kind == 'int64' else kind)
    if _is_torch(out) != on_dev:
        raise ValueError('out must be of the same kind as %s (numpy array or CUDA tensor)' % name)
    if on_dev:
        import torch
        ok = out.is_cuda and out.is_contiguous() and (
            out.element_size() == 8 and not out.is_floating_point() if kind == 'int64'
            else out.dtype == getattr(torch, kind))
    else:
        ok = isinstance(out, np.ndarray) and out.flags.c_contiguous and \
            out.dtype in ((np.uint64, np.int64) if kind == 'int64' else (np.dtype(kind),))
    if ok and isinstance(oshape, int):
        ok = int(out.numel() if on_dev else out.size) == oshape
    elif ok:
        ok = tuple(out.shape) == tuple(oshape)
    if not ok:
        raise ValueError('out must be a contiguous %s array of %s' % (
            '64-bit integer' if kind == 'int64' else kind, what or 'the shape of the box %s' % (oshape,)))
    return out


def _check_offsets(offsets):
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int32).reshape(-1, 3))
    if off.shape[0] > L.CTG_MAX_CHANNELS:
        raise ValueError('at most %d affinity channels are supported' % L.CTG_MAX_CHANNELS)
    return off


def rag_features_handle(labels, data=None, offsets=None, own_begin=None, own_end=None, ignore_label=False,
                        hist_range=(0.0, 1.0), keep_stats=False, stream=None, no_adj_filter=False,
                        defer_stats=False):
    """Run the hot path and return the device-resident ``Result`` handle.

    labels: (Z,Y,X) uint64/uint32 numpy array or CUDA tensor (int64/int32 views
    of unsigned labels are accepted for torch); data: None, (Z,Y,X) boundary
    map or (C,Z,Y,X) affinities (float32 or uint8); offsets: C x 3 for
    affinities.  keep_stats keeps the mergeable wide records; no_adj_filter
    (affinities) keeps sampled pairs that are not edges of this array's RAG;
    defer_stats (with keep_stats, for the multi-GPU exchange only:
    CTG_DEFER_STATS) writes no statistics rows -- the exchange rebuilds the
    rows it needs from this call's records, valid until the next call.
    """
    on_dev = _is_torch(labels)
    if on_dev:
        import torch
        assert labels.is_cuda and labels.is_contiguous(), 'labels must be a contiguous CUDA tensor'
        label_bits = labels.element_size() * 8
        shape = tuple(labels.shape)
        if data is not None:
            assert _is_torch(data) and data.is_cuda and data.is_contiguous()
            kind = L.CTG_DATA_U8 if data.dtype == torch.uint8 else L.CTG_DATA_F32
            if kind == L.CTG_DATA_F32:
                assert data.dtype == torch.float32
    else:
        labels = np.asarray(labels)
        if labels.dtype not in (np.uint64, np.uint32, np.int64, np.int32):
            labels = labels.astype(np.uint64)
        labels = np.ascontiguousarray(labels)
        label_bits = labels.dtype.itemsize * 8
        shape = labels.shape
        if data is not None:
            data = np.asarray(data)
            if data.dtype == np.uint8:
                kind = L.CTG_DATA_U8
            else:
                kind = L.CTG_DATA_F32
                data = data.astype(np.float32, copy=False)
            data = np.ascontiguousarray(data)
    if len(shape) != 3:
        raise ValueError('labels must be 3-D, got shape %s' % (shape,))
    n_ch = 0
    off_ptr = None
    off = None
    if data is None:
        kind = L.CTG_DATA_NONE
    elif offsets is not None:
        off = _check_offsets(offsets)
        n_ch = off.shape[0]
        if tuple(data.shape) != (n_ch,) + tuple(shape):
            raise ValueError('affinities must be (C,Z,Y,X) = %s, got %s' % ((n_ch,) + tuple(shape),
                                                                           tuple(data.shape)))
        off_ptr = off.ctypes.data_as(ctypes.c_void_p)
    else:
        if tuple(data.shape) != tuple(shape):
            raise ValueError('boundary map shape %s != labels shape %s' % (tuple(data.shape), tuple(shape)))
    flags = ((L.CTG_KEEP_STATS if keep_stats else 0) | (L.CTG_NO_ADJ_FILTER if no_adj_filter else 0) |
             (L.CTG_DEFER_STATS if keep_stats and defer_stats else 0))
    return _create(Result, 'ctg_rag_features', _ptr(labels), label_bits, _ptr(data), kind, n_ch, off_ptr,
                   _shape_arr(shape), _shape_arr(own_begin), _shape_arr(own_end), int(bool(ignore_label)),
                   float(hist_range[0]), float(hist_range[1]), flags, _mem(on_dev), _stream(stream, on_dev))


def rag_features(labels, data=None, offsets=None, own_begin=None, own_end=None, ignore_label=False,
                 hist_range=(0.0, 1.0), keep_stats=False, no_adj_filter=False):
    """Host convenience: returns dict(edges, nodes, features[, sums, records])."""
    with rag_features_handle(labels, data, offsets, own_begin, own_end, ignore_label, hist_range, keep_stats,
                             no_adj_filter=no_adj_filter) as r:
        out = dict(edges=r.edges(), nodes=r.nodes())
        if data is not None:
            out['features'] = r.features()
            if keep_stats:
                out['sums'], out['records'] = r.stats()
        return _with_info(r, out)


def _with_info(r, out):
    out['n_records'], out['n_direct'] = r.info()
    return out


_arena_pool = []
_arena_lock = threading.Lock()
ARENA_POOL_BYTES = 8 << 30


def _leak_arenas_at_exit():
    """Interpreter exit: drop the pooled page-locked arenas without unpinning
    them one by one (hipHostFree ~0.2 s per GB in a drop-in job process that
    is about to end; process teardown releases the pages).  CTG_EXIT_FREE=1
    keeps the explicit frees."""
    import os
    if os.environ.get('CTG_EXIT_FREE') == '1':
        return
    with _arena_lock:
        for a in _arena_pool:
            a.ptr = None
        _arena_pool.clear()


import atexit  # noqa: E402
atexit.register(_leak_arenas_at_exit)


def host_arena(nbytes):
    """A page-locked arena of at least ``nbytes`` from the process pool
    (pinning GBs of host memory costs ~0.2 s/GB: arenas are kept for the next
    batch / call); give it back with release_arena."""
    with _arena_lock:
        best = None
        for a in _arena_pool:
            if a.nbytes >= nbytes and (best is None or a.nbytes < best.nbytes):
                best = a
        if best is not None:
            _arena_pool.remove(best)
            return best
    return HostArena(nbytes)


def release_arena(arena):
    with _arena_lock:
        _arena_pool.append(arena)
        _arena_pool.sort(key=lambda a: -a.nbytes)
        while sum(a.nbytes for a in _arena_pool) > ARENA_POOL_BYTES and len(_arena_pool) > 1:
            _arena_pool.pop().free()


class HostArena:
    """Page-locked host buffer (ctg_host_alloc) viewed as a numpy array: the
    staging area of batched block inputs (decoded N5 ROIs go straight in)."""

    def __init__(self, nbytes):
        self.nbytes = int(max(nbytes, 64))
        lib = L.load()
        L.init_device()
        self.ptr = lib.ctg_host_alloc(self.nbytes)
        if not self.ptr:
            L.check(-3, 'ctg_host_alloc')
        self.buf = (ctypes.c_char * self.nbytes).from_address(self.ptr)

    def view(self, dtype, count, offset_bytes=0):
        return np.frombuffer(self.buf, dtype=dtype, count=int(count), offset=int(offset_bytes))

    def free(self):
        if getattr(self, 'ptr', None):
            L.load().ctg_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        self.free()


def _desc(blocks):
    arr = (L.BlockDesc * len(blocks))()
    for d, b in zip(arr, blocks):
        d.label_offset = int(b['label_offset'])
        d.data_offset = int(b.get('data_offset', 0))
        for k in range(3):
            d.shape[k] = int(b['shape'][k])
            d.own_begin[k] = int(b['own'][0][k])
            d.own_end[k] = int(b['own'][1][k])
            d.graph_begin[k] = int(b['graph'][0][k])
            d.graph_end[k] = int(b['graph'][1][k])
    return arr


def rag_blocks_arena(labels, blocks, data=None, offsets=None, ignore_label=False, hist_range=(0.0, 1.0),
                     keep_stats=False, nodes=True, stream=None):
    """ctg_rag_blocks over arenas that already hold the block arrays.

    labels: 1-D uint64/uint32 array (host, ideally a HostArena view);
    data: None or 1-D float32/uint8 array; blocks: list of dicts with
    label_offset, data_offset, shape, own=(begin, end), graph=(begin, end).
    Returns one dict per block: nodes, edges[, features, sums, records]."""
    on_dev = _is_torch(labels)
    if on_dev:   # device-resident arenas (torch CUDA tensors, int64/int32 views of the labels)
        import torch
        assert labels.is_cuda and labels.is_contiguous() and labels.element_size() in (4, 8)
        label_bits = labels.element_size() * 8
        n_lab = labels.numel()
        if data is not None:
            assert _is_torch(data) and data.is_cuda and data.is_contiguous()
            assert data.dtype in (torch.float32, torch.uint8)
    else:
        labels = np.asarray(labels)
        if labels.dtype not in (np.uint64, np.uint32):
            raise ValueError('labels arena must be uint64 or uint32')
        label_bits = labels.dtype.itemsize * 8
        n_lab = labels.size
    kind = L.CTG_DATA_NONE
    n_ch = 0
    off_ptr = None
    n_dat = 0
    if data is not None:
        if on_dev:
            import torch
            kind = L.CTG_DATA_U8 if data.dtype == torch.uint8 else L.CTG_DATA_F32
            n_dat = data.numel()
        else:
            data = np.asarray(data)
            kind = L.CTG_DATA_U8 if data.dtype == np.uint8 else L.CTG_DATA_F32
            if kind == L.CTG_DATA_F32 and data.dtype != np.float32:
                raise ValueError('data arena must be float32 or uint8')
            n_dat = data.size
        if offsets is not None:
            off = _check_offsets(offsets)
            n_ch = off.shape[0]
            off_ptr = off.ctypes.data_as(ctypes.c_void_p)
    desc = _desc(blocks)
    flags = (L.CTG_KEEP_STATS if keep_stats else 0) | (0 if nodes else L.CTG_NO_NODES)
    nb = len(blocks)
    eoff = np.zeros(nb + 1, np.int64)
    noff = np.zeros(nb + 1, np.int64)
    with _create(Result, 'ctg_rag_blocks', _ptr(labels), label_bits, _ptr(data), kind, n_ch, off_ptr,
                 ctypes.cast(desc, ctypes.c_void_p), nb, n_lab, n_dat, int(bool(ignore_label)),
                 float(hist_range[0]), float(hist_range[1]), flags, _mem(on_dev), _stream(stream, on_dev)) as r:
        L.check(L.load().ctg_result_block_offsets(r.handle, _ptr(eoff), _ptr(noff)), 'ctg_result_block_offsets')
        edges, nodes = r.edges(), r.nodes()
        feats = r.features() if data is not None else None
        sums = recs = None
        if keep_stats and data is not None:
            sums, recs = r.stats()
    out = []
    for b in range(nb):
        e0, e1, n0, n1 = eoff[b], eoff[b + 1], noff[b], noff[b + 1]
        d = dict(edges=edges[e0:e1], nodes=nodes[n0:n1])
        if feats is not None:
            d['features'] = feats[e0:e1]
        if sums is not None:
            d['sums'], d['records'] = sums[e0:e1], recs[e0:e1]
        out.append(d)
    return out


def rag_blocks(arrays, own, graph, data=None, offsets=None, ignore_label=False, hist_range=(0.0, 1.0),
               keep_stats=False, stream=None):
    """Convenience front end of rag_blocks_arena: per-block label arrays
    (and data arrays: (Z,Y,X) boundary maps or (C,Z,Y,X) affinities) with
    their own / graph boxes ((begin, end) in array coordinates)."""
    lab = [np.ascontiguousarray(np.asarray(a)) for a in arrays]
    dt = np.uint32 if all(a.dtype == np.uint32 for a in lab) else np.uint64
    lab_arena = np.concatenate([a.astype(dt, copy=False).ravel() for a in lab]) if lab else np.zeros(0, dt)
    blocks, lo, do = [], 0, 0
    dat_arena = None
    if data is not None:
        dd = [np.ascontiguousarray(np.asarray(x)) for x in data]
        ddt = np.uint8 if all(x.dtype == np.uint8 for x in dd) else np.float32
        dat_arena = np.concatenate([x.astype(ddt, copy=False).ravel() for x in dd])
    for i, a in enumerate(lab):
        blocks.append(dict(label_offset=lo, data_offset=do, shape=a.shape, own=own[i], graph=graph[i]))
        lo += a.size
        if data is not None:
            do += data[i].size
    return rag_blocks_arena(lab_arena, blocks, dat_arena, offsets, ignore_label, hist_range, keep_stats,
                            stream=stream)


def unique_labels(labels, begin=None, end=None, stream=None):
    """Sorted unique labels of labels[begin:end] (uint64 numpy array)."""
    on_dev = _is_torch(labels)
    if not on_dev:
        labels = np.ascontiguousarray(np.asarray(labels).astype(np.uint64, copy=False))
    with _create(Result, 'ctg_unique_labels', _ptr(labels), _shape_arr(tuple(labels.shape)), _shape_arr(begin),
                 _shape_arr(end), _mem(on_dev), _stream(stream, on_dev)) as r:
        return r.nodes()


def merge_stats_handle(keys, sums, records, hist_range=(0.0, 1.0), keep_stats=False, stream=None):
    """Device-resident merge of partial statistics: keys (n,2), sums (n,2)
    float64, records (n,48) 32-bit words; numpy (host) or CUDA tensors."""
    on_dev = _is_torch(keys)
    if on_dev:
        for t in (keys, sums, records):
            assert _is_torch(t) and t.is_cuda and t.is_contiguous(), 'merge inputs must be contiguous CUDA tensors'
        n = keys.shape[0]
        assert keys.element_size() == 8 and keys.numel() == 2 * n
        assert sums.element_size() == 8 and sums.numel() == 2 * n
        assert records.element_size() == 4 and records.numel() == WIDE_WORDS * n
    else:
        keys = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64).reshape(-1, 2))
        sums = np.ascontiguousarray(np.asarray(sums, dtype=np.float64).reshape(-1, 2))
        records = np.ascontiguousarray(np.asarray(records, dtype=np.uint32).reshape(-1, WIDE_WORDS))
        n = keys.shape[0]
        assert sums.shape[0] == n and records.shape[0] == n
    return _create(Result, 'ctg_merge_stats', _ptr(keys), _ptr(sums), _ptr(records), n, float(hist_range[0]),
                   float(hist_range[1]), int(bool(keep_stats)), _mem(on_dev), _stream(stream, on_dev))


def unique_values_handle(values, stream=None):
    """Sorted unique values of a uint64 list (numpy or CUDA int64 tensor) -> Result (nodes)."""
    on_dev = _is_torch(values)
    if not on_dev:
        values = np.ascontiguousarray(np.asarray(values, dtype=np.uint64).reshape(-1))
    else:
        assert values.is_cuda and values.is_contiguous() and values.element_size() == 8
    return _create(Result, 'ctg_unique_values', _ptr(values), int(values.shape[0]), _mem(on_dev),
                   _stream(stream, on_dev))


def merge_stats(keys, sums, records, hist_range=(0.0, 1.0), keep_stats=False):
    """Combine partial statistics tables (wide records) -> dict(edges, features[, sums, records])."""
    with merge_stats_handle(keys, sums, records, hist_range, keep_stats) as r:
        out = dict(edges=r.edges(), features=r.features())
        if keep_stats:
            out['sums'], out['records'] = r.stats()
    return out


def merge_feature_rows(ids, rows, id_begin, id_end, stream=None):
    """Reference-layout (n,10) feature rows of global edge ids -> the merged
    (id_end - id_begin, 10) rows (ctg_merge_feature_rows)."""
    lib = L.load()
    L.init_device()
    ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64).reshape(-1))
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, N_FEATURES))
    if rows.shape[0] != ids.shape[0]:
        raise ValueError('ids and rows differ in length')
    out = np.zeros((int(id_end) - int(id_begin), N_FEATURES), dtype=np.float64)
    L.check(lib.ctg_merge_feature_rows(_ptr(ids), _ptr(rows), ids.shape[0], int(id_begin), int(id_end), _ptr(out),
                                       L.CTG_MEM_HOST, stream), 'ctg_merge_feature_rows')
    return out


def unique_pairs(pairs, stream=None):
    """Sorted unique rows of an (n,2) uint64 pair list -> (edges, nodes)."""
    p = np.ascontiguousarray(np.asarray(pairs, dtype=np.uint64).reshape(-1, 2))
    with _create(Result, 'ctg_unique_pairs', _ptr(p), p.shape[0], L.CTG_MEM_HOST, stream) as r:
        return r.edges(), r.nodes()


def map_edge_ids(global_edges, query, stream=None):
    """Row of every query (u,v) in the sorted global edge table (-1 if absent)."""
    lib = L.load()
    L.init_device()
    g = np.ascontiguousarray(np.asarray(global_edges, dtype=np.uint64).reshape(-1, 2))
    q = np.ascontiguousarray(np.asarray(query, dtype=np.uint64).reshape(-1, 2))
    out = np.empty(q.shape[0], dtype=np.int64)
    rc = lib.ctg_map_edge_ids(_ptr(g), g.shape[0], _ptr(q), q.shape[0], _ptr(out), L.CTG_MEM_HOST, stream)
    L.check(rc, 'ctg_map_edge_ids')
    return out


def _label_volume(x, name):
    """A label volume argument -> (array, bits): a contiguous CUDA tensor as it
    is, anything else as a C-contiguous numpy array of 32- or 64-bit labels."""
    if _is_torch(x):
        if not (x.is_cuda and x.is_contiguous()) or x.element_size() not in (4, 8) or x.is_floating_point():
            raise ValueError('%s must be a contiguous CUDA tensor of 32- or 64-bit integers' % name)
        return x, x.element_size() * 8
    x = np.asarray(x)
    if x.dtype.kind not in 'ui':
        raise TypeError('%s must hold integer labels, got %s' % (name, x.dtype))
    if x.dtype not in (np.uint64, np.uint32, np.int64, np.int32):
        x = x.astype(np.uint64)
    return np.ascontiguousarray(x), x.dtype.itemsize * 8


def _data_volume(x, on_dev):
    """A data volume argument (of the caller's kind: ``on_dev``) -> (array, CTG_DATA_*): float32 or uint8."""
    if on_dev:
        import torch
        if not (x.is_cuda and x.is_contiguous()) or x.dtype not in (torch.float32, torch.uint8):
            raise ValueError('data must be a contiguous float32 or uint8 CUDA tensor')
        return x, L.CTG_DATA_U8 if x.dtype == torch.uint8 else L.CTG_DATA_F32
    x = np.asarray(x)
    if x.dtype not in (np.float32, np.uint8):
        raise TypeError('data must be float32 or uint8, got %s' % x.dtype)
    return np.ascontiguousarray(x), L.CTG_DATA_U8 if x.dtype == np.uint8 else L.CTG_DATA_F32


def _volume_call(fn, labels, second, name, triples, ignore_label, stream):
    """The three calls that scan a label volume -> their ``Result``: lib.<fn>(labels, bits[, second, its code],
    shape, *triples[, whether to ignore, ignore_label], mem, stream).  ``second``: the ``values`` to overlap
    with, the ``data`` to accumulate, or no second volume (``name`` None, and no ignore label then).  A triple
    that is None stays a null pointer: the library does the defaulting and the range check."""
    if name and _is_torch(labels) != _is_torch(second):
        raise ValueError('labels and %s must both be numpy arrays or both CUDA tensors' % name)
    labels, bits = _label_volume(labels, 'labels')
    on_dev = _is_torch(labels)
    args = [_ptr(labels), bits]
    if name:
        second, code = _label_volume(second, name) if name == 'values' else _data_volume(second, on_dev)
        args += [_ptr(second), code]
    shape = tuple(labels.shape)
    if len(shape) != 3:
        raise ValueError('labels must be 3-D, got shape %s' % (shape,))
    if name and tuple(second.shape) != shape:
        raise ValueError('%s shape %s != labels shape %s' % (name, tuple(second.shape), shape))
    if any(t is not None and len(t) != 3 for t in triples):
        raise ValueError('%s must have 3 entries' % ' / '.join(('begin', 'end', 'origin')[:len(triples)]))
    if ignore_label is not None and not 0 <= int(ignore_label) < 1 << 64:
        raise ValueError('ignore_label must be a uint64 value or None, got %r' % (ignore_label,))
    ignore = [int(ignore_label is not None), int(ignore_label or 0)] if name else []
    return _create(Result, fn, *args, _shape_arr(shape), *[_shape_arr(t) for t in triples], *ignore, _mem(on_dev),
                   _stream(stream, on_dev))


def label_overlaps_handle(labels, values, begin=None, end=None, ignore_label=None, stream=None):
    """ctg_label_overlaps -> the device-resident ``Result``: edges() = the
    distinct (labels[p], values[p]) pairs of the box [begin, end), sorted;
    counts() = their voxel counts; nodes() = the distinct labels.  Voxels whose
    *value* equals ``ignore_label`` are skipped (None: every voxel counts,
    zeros included).  Both volumes numpy arrays or both CUDA tensors, (Z,Y,X),
    32- or 64-bit integers."""
    return _volume_call('ctg_label_overlaps', labels, values, 'values', (begin, end), ignore_label, stream)


def _overlap_tables(r):
    return dict(pairs=r.edges(), counts=r.counts(), nodes=r.nodes())


def label_overlaps(labels, values, begin=None, end=None, ignore_label=None):
    """Host convenience of label_overlaps_handle: dict(pairs (E,2), counts (E,),
    nodes (N,)) as uint64 numpy arrays (+ n_records, n_direct)."""
    with label_overlaps_handle(labels, values, begin, end, ignore_label) as r:
        return _with_info(r, _overlap_tables(r))


def merge_overlaps_handle(pairs, counts, stream=None):
    """ctg_merge_overlaps: rows (a, b) with counts, in any order -> the sorted
    table in which equal pairs have added their counts (``Result``)."""
    on_dev = _is_torch(pairs)
    if on_dev != _is_torch(counts):
        raise ValueError('pairs and counts must both be numpy arrays or both CUDA tensors')
    if on_dev:
        for t in (pairs, counts):
            if not (t.is_cuda and t.is_contiguous()) or t.element_size() != 8 or t.is_floating_point():
                raise ValueError('merge inputs must be contiguous 64-bit integer CUDA tensors')
        n = int(counts.numel())
        if int(pairs.numel()) != 2 * n:
            raise ValueError('%d pair entries for %d counts' % (int(pairs.numel()), n))
    else:
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.uint64).reshape(-1, 2))
        counts = np.ascontiguousarray(np.asarray(counts, dtype=np.uint64).reshape(-1))
        n = counts.shape[0]
        if pairs.shape[0] != n:
            raise ValueError('%d pairs for %d counts' % (pairs.shape[0], n))
    return _create(Result, 'ctg_merge_overlaps', _ptr(pairs), _ptr(counts), n, _mem(on_dev), _stream(stream, on_dev))


def merge_overlaps(pairs, counts):
    """Host convenience of merge_overlaps_handle: dict(pairs, counts, nodes)."""
    with merge_overlaps_handle(pairs, counts) as r:
        return _overlap_tables(r)


def _label_range(label_begin, label_end):
    lb, le = int(label_begin), int(label_end)
    if lb < 0 or le < lb:
        raise ValueError('need 0 <= label_begin <= label_end, got [%d, %d)' % (lb, le))
    return lb, le


def _read_dense(handle_or_tables, merge, keys, stream, fn, *args):
    """The dense-table readers: lib.<fn>(handle, *args, host memory, stream) on ``handle_or_tables`` -- a
    ``Result`` as it is, or a dict whose ``keys`` go through ``merge`` first; that handle ends here."""
    if isinstance(handle_or_tables, Result):
        scope = contextlib.nullcontext(handle_or_tables)
    else:
        scope = merge(*[handle_or_tables[k] for k in keys], stream)
    with scope as r:
        L.check(getattr(L.load(), fn)(r.handle, *args, L.CTG_MEM_HOST, _handle_stream(stream)), fn)


def max_overlaps(handle_or_tables, label_begin, label_end, stream=None):
    """Per label in [label_begin, label_end) the value it overlaps most and
    that overlap: (labels, counts), uint64 arrays of label_end - label_begin
    entries, 0 / 0 for labels without a row; equal counts go to the smallest
    value.  ``handle_or_tables``: a ``Result`` of label_overlaps_handle /
    merge_overlaps_handle, or a dict with 'pairs' and 'counts' (merged first)."""
    lb, le = _label_range(label_begin, label_end)
    out_l = np.zeros(le - lb, dtype=np.uint64)
    out_c = np.zeros(le - lb, dtype=np.uint64)
    _read_dense(handle_or_tables, merge_overlaps_handle, ('pairs', 'counts'), stream, 'ctg_max_overlaps', lb, le,
                _ptr(out_l), _ptr(out_c))
    return out_l, out_c


def morphology_handle(labels, begin=None, end=None, origin=None, stream=None):
    """ctg_morphology -> the device-resident ``Result``: nodes() = the distinct
    labels of the box [begin, end), ascending; moments() = their (N,10) uint64
    table [n, sum z y x, min z y x, max z y x] (max inclusive); morph_rows() =
    the float64 rows [id, size, com z y x, min z y x, max z y x].  The
    coordinate of the voxel at array index p is p + ``origin`` (the block's
    begin when ``labels`` is one block of a volume).  A numpy array or a CUDA
    tensor, (Z,Y,X), 32- or 64-bit integers; label 0 is a label like any other."""
    return _volume_call('ctg_morphology', labels, None, None, (begin, end, origin), None, stream)


def _morphology_tables(r):
    return dict(nodes=r.nodes(), moments=r.moments(), rows=r.morph_rows())


def morphology(labels, begin=None, end=None, origin=None):
    """Host convenience of morphology_handle: dict(nodes (N,) uint64, moments
    (N,10) uint64, rows (N,11) float64, n_records, n_direct).  A label of 2^53
    or more does not fit the rows' id column: use the handle's nodes() and
    moments() for such volumes."""
    with morphology_handle(labels, begin, end, origin) as r:
        return _with_info(r, _morphology_tables(r))


def _merge_rows(fn, rows, cols, noun, stream):
    """The two merges of float64 row tables -> their ``Result``: lib.<fn>(rows, their number, mem, stream)."""
    on_dev = _is_torch(rows)
    if on_dev:
        if not (rows.is_cuda and rows.is_contiguous()) or rows.element_size() != 8 or not rows.is_floating_point():
            raise ValueError('rows must be a contiguous float64 CUDA tensor')
        size = int(rows.numel())
    else:
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float64))
        size = rows.size
    if size % cols or (size and rows.ndim == 2 and rows.shape[1] != cols):
        raise ValueError('%s rows have %d columns, got %s' % (noun, cols, tuple(rows.shape)))
    return _create(Result, fn, _ptr(rows), size // cols, _mem(on_dev), _stream(stream, on_dev))


def merge_morphology_handle(rows, stream=None):
    """ctg_merge_morphology: (n,11) float64 rows of partial tables, in any
    order -> the table in which the rows of one id are combined (``Result``):
    sizes add, boxes fold, and the coordinate sums add as integers, so the
    result equals one morphology call over the whole volume while every row's
    sum is below 2^51."""
    return _merge_rows('ctg_merge_morphology', rows, MORPH_COLS, 'morphology', stream)


def merge_morphology(rows):
    """Host convenience of merge_morphology_handle: dict(nodes, moments, rows)."""
    with merge_morphology_handle(rows) as r:
        return _morphology_tables(r)


def morphology_rows(handle_or_tables, label_begin, label_end, stream=None):
    """The dense (label_end - label_begin, 11) float64 table of the labels in
    [label_begin, label_end): the row of label a at a - label_begin, zeros for
    absent labels.  ``handle_or_tables``: a ``Result`` of morphology_handle /
    merge_morphology_handle, or a dict with 'rows' (merged first)."""
    lb, le = _label_range(label_begin, label_end)
    out = np.zeros((le - lb, MORPH_COLS), dtype=np.float64)
    _read_dense(handle_or_tables, merge_morphology_handle, ('rows',), stream, 'ctg_morphology_rows', lb, le,
                _ptr(out), None)
    return out


def region_features_handle(labels, data, begin=None, end=None, ignore_label=None, stream=None):
    """ctg_region_features -> the device-resident ``Result``: nodes() = the
    distinct labels of the box [begin, end), ascending; region_moments() = their
    voxel counts and the sums, minima and maxima of ``data`` over their voxels;
    region_rows() = the float64 rows of either form.  Voxels whose *label*
    equals ``ignore_label`` are not counted and that label gets no row (None:
    every voxel counts, label 0 included).  Both volumes numpy arrays or both
    CUDA tensors, (Z,Y,X); labels 32- or 64-bit integers, data float32 or uint8
    (a channel of a 4-D input: pass ``data[channel]``)."""
    return _volume_call('ctg_region_features', labels, data, 'data', (begin, end), ignore_label, stream)


def _region_tables(r, norm):
    counts, sums, minmax = r.region_moments()
    return dict(nodes=r.nodes(), counts=counts, sums=sums, minmax=minmax, rows=r.region_rows('sums'),
                features=r.region_rows('features', norm))


def region_norm(data):
    """What the samples of ``data`` are divided by unless the caller says otherwise: 255 for uint8, else 1
    (region_features.py:151-157)."""
    return 255.0 if str(data.dtype).endswith('uint8') else 1.0


def region_features(labels, data, begin=None, end=None, ignore_label=None, norm=None):
    """Host convenience of region_features_handle: dict(nodes (N,) uint64,
    counts (N,) uint64, sums (N,) float64, minmax (N,2) float32, rows (N,5)
    float64 in the sum form, features (N,5) float64 in the feature form over
    ``norm`` -- None: 255 for uint8 data and 1 otherwise -- n_records,
    n_direct).  A label of 2^53 or more does not fit the rows' id column: use
    the handle's nodes() and region_moments() for such volumes."""
    if norm is None:
        norm = region_norm(data)
    with region_features_handle(labels, data, begin, end, ignore_label) as r:
        return _with_info(r, _region_tables(r, norm))


def merge_region_features_handle(rows, stream=None):
    """ctg_merge_region_features: (n,5) float64 rows [id, count, sum, min, max]
    of partial tables, in any order -> the table in which the rows of one id
    are combined (``Result``): counts and sums add, min and max fold."""
    return _merge_rows('ctg_merge_region_features', rows, REGION_COLS, 'region-feature', stream)


def merge_region_features(rows, norm=1.0):
    """Host convenience of merge_region_features_handle: the dict of region_features."""
    with merge_region_features_handle(rows) as r:
        return _region_tables(r, norm)


def region_feature_rows(handle_or_tables, label_begin, label_end, form='features', norm=1.0, stream=None):
    """The dense (label_end - label_begin, 5) float64 table of the labels in
    [label_begin, label_end) in ``form`` ('features': [id, count, mean, minimum,
    maximum] over ``norm``; 'sums': [id, count, sum, min, max]): the row of
    label a at a - label_begin, zeros for absent labels.  ``handle_or_tables``:
    a ``Result`` of region_features_handle / merge_region_features_handle, or a
    dict with 'rows' in the sum form (merged first)."""
    lb, le = _label_range(label_begin, label_end)
    code = _region_form(form)
    if not (float(norm) > 0.0 and float(norm) < float('inf')):
        raise ValueError('norm must be finite and positive, got %r' % (norm,))
    out = np.zeros((le - lb, REGION_COLS), dtype=np.float64)
    _read_dense(handle_or_tables, merge_region_features_handle, ('rows',), stream, 'ctg_region_rows', lb, le, code,
                float(norm), _ptr(out), None)
    return out


class Assignment(_Handle):
    """Owning wrapper around a ``ctg_assignment*`` handle: a node assignment in
    device memory (assignment_dense, assignment_sparse), uploaded once and
    applied to any number of label arrays (apply_assignment)."""
    _free = 'ctg_assignment_free'

    def __init__(self, handle, device):
        super().__init__(handle, device)
        n, mx, kind = ctypes.c_int64(), ctypes.c_uint64(), ctypes.c_int()
        L.check(L.load().ctg_assignment_info(handle, ctypes.byref(n), ctypes.byref(mx), ctypes.byref(kind)),
                'ctg_assignment_info')
        self.n = int(n.value)                   # entries of a dense table / pairs of a sparse one
        self.max_value = int(mx.value)          # the largest value (0: empty)
        self.kind = 'sparse' if kind.value == L.CTG_ASSIGN_SPARSE else 'dense'


def _u64_vector(x, name):
    """A 1-D table argument -> (array, on_device): a contiguous 64-bit integer
    CUDA tensor as it is, anything else as a contiguous uint64 numpy array."""
    if _is_torch(x):
        if not (x.is_cuda and x.is_contiguous()) or x.element_size() != 8 or x.is_floating_point() or x.dim() != 1:
            raise ValueError('%s must be a contiguous 1-D CUDA tensor of 64-bit integers' % name)
        return x, True
    x = np.asarray(x)
    if x.dtype.kind not in 'ui' and x.size:
        raise TypeError('%s must hold integers, got %s' % (name, x.dtype))
    if x.ndim != 1:
        raise ValueError('%s must be 1-D, got shape %s' % (name, x.shape))
    if x.dtype.kind == 'i' and x.size and int(x.min()) < 0:
        raise ValueError('%s holds negative values' % name)
    return np.ascontiguousarray(x, dtype=np.uint64), False


def assignment_dense(table, stream=None):
    """ctg_assignment_dense: A(l) = table[l] (what nifty.tools.take indexes);
    labels of len(table) and above are out of range."""
    table, on_dev = _u64_vector(table, 'table')
    return _create(Assignment, 'ctg_assignment_dense', _ptr(table), int(table.shape[0]), _mem(on_dev),
                   _stream(stream, on_dev))


def assignment_sparse(keys, values, stream=None):
    """ctg_assignment_sparse: A(keys[i]) = values[i] (the dict that
    nifty.tools.takeDict reads), keys in any order.  A key given twice is an
    error; 0 is a key like any other."""
    keys, on_dev = _u64_vector(keys, 'keys')
    values, v_dev = _u64_vector(values, 'values')
    if on_dev != v_dev:
        raise ValueError('keys and values must both be numpy arrays or both CUDA tensors')
    if keys.shape[0] != values.shape[0]:
        raise ValueError('%d keys for %d values' % (keys.shape[0], values.shape[0]))
    return _create(Assignment, 'ctg_assignment_sparse', _ptr(keys), _ptr(values), int(keys.shape[0]), _mem(on_dev),
                   _stream(stream, on_dev))


def apply_assignment(a, labels, offset=0, segments=None, allow_missing=False, out=None, check_only=False, stream=None):
    """ctg_apply_assignment: out[i] = A(labels[i] + off) with zeros unshifted,
    over the flattened (C-order) ``labels`` -- a numpy array or a CUDA tensor of
    32- or 64-bit integers, of any shape.

    ``offset``: the label offset of the whole array; or ``segments`` =
    (seg_begin, seg_offset): segment k is the flat range [seg_begin[k],
    seg_begin[k + 1]) with its own offset (the blocks of a job in one call).
    ``out``: None (a new uint64 array / int64 tensor of the labels' shape), an
    array of the same kind and size, or ``labels`` itself (in place, 64-bit
    labels).  ``check_only``: nothing is written, the counts alone.
    A label without an entry raises KeyError (sparse) or IndexError (dense)
    naming the smallest one, unless ``allow_missing`` (sparse only): such voxels
    then keep their shifted label.

    Returns (out, info): out is None with ``check_only``; info = dict(nonzero =
    the nonzero input voxels per segment (uint64 array; one entry without
    segments), n_missing, first_missing (None if none))."""
    if not isinstance(a, Assignment) or not a.handle:
        raise TypeError('a must be a live Assignment')
    labels, bits = _label_volume(labels, 'labels')
    on_dev = _is_torch(labels)
    n = int(labels.numel()) if on_dev else int(labels.size)
    if segments is not None:
        if offset:
            raise ValueError('give offset or segments, not both')
        seg_begin = np.ascontiguousarray(np.asarray(segments[0], dtype=np.int64).reshape(-1))
        seg_off = np.ascontiguousarray(np.asarray(segments[1], dtype=np.uint64).reshape(-1))
        if seg_begin.shape[0] != seg_off.shape[0] + 1:
            raise ValueError('segments: %d begins for %d offsets (need one more)' % (seg_begin.shape[0], seg_off.shape[0]))
        n_seg = int(seg_off.shape[0])
    else:
        if not 0 <= int(offset) < 1 << 64:
            raise ValueError('offset must be a uint64 value, got %r' % (offset,))
        seg_begin = np.array([0, n], dtype=np.int64)
        seg_off = np.array([int(offset)], dtype=np.uint64)
        n_seg = 1
    if allow_missing and a.kind != 'sparse':
        raise ValueError('allow_missing needs a sparse assignment')
    if check_only:
        if out is not None:
            raise ValueError('check_only writes nothing: out must be None')
    elif out is None:
        out = _dense_out(None, tuple(labels.shape), on_dev, labels, 'int64', 'labels')
    else:
        _dense_out(out, n, on_dev, labels, 'int64', 'labels', 'the size of labels')
        if bits != 64 and _ptr(out).value == _ptr(labels).value and n:
            raise ValueError('in place needs 64-bit labels')
    lib = L.load()
    L.init_device()
    nonzero = np.zeros(max(n_seg, 1), dtype=np.uint64)
    missing = np.zeros(2, dtype=np.uint64)
    rc = lib.ctg_apply_assignment(a.handle, _ptr(labels), bits, n, _ptr(seg_begin), _ptr(seg_off), n_seg,
                                  int(bool(allow_missing)), _ptr(out), _ptr(nonzero), _ptr(missing),
                                  _mem(on_dev), _stream(stream, on_dev))
    if rc == L.CTG_ERR_MISSING:
        msg = '%d: the smallest of the labels without an entry (%d voxel(s))' % (int(missing[1]), int(missing[0]))
        if a.kind == 'sparse':
            raise KeyError(msg)
        raise IndexError(msg + '; the table has %d entries' % a.n)
    L.check(rc, 'ctg_apply_assignment')
    info = dict(nonzero=nonzero[:n_seg], n_missing=int(missing[0]),
                first_missing=int(missing[1]) if missing[0] else None)
    return out, info


CC_MODES = {'greater': L.CTG_CC_GREATER, 'less': L.CTG_CC_LESS, 'equal': L.CTG_CC_EQUAL}


def threshold_components(data, threshold, mode='greater', mask=None, normalize=True, connectivity=3, begin=None,
                         end=None, out=None, stream=None):
    """ctg_threshold_components: the connected components of the thresholded
    box [begin, end) of ``data`` -> (labels, n).

    ``data``: a (Z,Y,X) numpy array or contiguous CUDA tensor, float32 or uint8.
    A voxel is foreground where ``v > threshold`` / ``v < threshold`` /
    ``v == threshold`` (``mode`` 'greater', 'less', 'equal', in float32) and,
    with a ``mask`` (same shape and kind as data, bool or uint8), the mask is
    nonzero.  ``v`` is the sample, or with ``normalize`` the value of
    vu.normalize over the box (utils/volume_utils.py:98-105); a NaN in a
    normalised box gives the empty result, as numpy's minimum does.
    ``connectivity`` 1, 2, 3: 6, 18 or 26 neighbours (skimage's label on a
    boolean array: 3).  ``labels``: box-shaped uint64 (an int64 tensor for
    tensors; ``out`` to write into an existing one), 0 for the background, the
    components numbered 1 .. n in raster order of their first voxels, which is
    scipy.ndimage.label's numbering."""
    if mode not in CC_MODES:
        raise ValueError("mode must be 'greater', 'less' or 'equal', got %r" % (mode,))
    if connectivity not in (1, 2, 3):
        raise ValueError('connectivity must be 1, 2 or 3, got %r' % (connectivity,))
    on_dev = _is_torch(data)
    data, kind = _data_volume(data, on_dev)
    shape = tuple(data.shape)
    if len(shape) != 3:
        raise ValueError('data must be 3-D, got shape %s' % (shape,))
    if mask is not None:
        if _is_torch(mask) != on_dev:
            raise ValueError('data and mask must both be numpy arrays or both CUDA tensors')
        if tuple(mask.shape) != shape:
            raise ValueError('mask shape %s != data shape %s' % (tuple(mask.shape), shape))
        if on_dev:
            import torch
            if mask.dtype == torch.bool:
                mask = mask.to(torch.uint8)
            if not (mask.is_cuda and mask.is_contiguous()) or mask.dtype != torch.uint8:
                raise ValueError('mask must be a contiguous bool or uint8 CUDA tensor')
        else:
            mask = np.asarray(mask)
            if mask.dtype not in (np.bool_, np.uint8):
                raise TypeError('mask must be bool or uint8, got %s' % mask.dtype)
            mask = np.ascontiguousarray(mask).view(np.uint8)
    b, e, oshape = _box(shape, begin, end)
    out = _dense_out(out, oshape, on_dev, data, 'int64', 'data')
    lib = L.load()
    L.init_device()
    n = ctypes.c_uint64(0)
    rc = lib.ctg_threshold_components(_ptr(data), kind, _ptr(mask), _shape_arr(shape), _shape_arr(b), _shape_arr(e),
                                      float(threshold), CC_MODES[mode], int(bool(normalize)), int(connectivity),
                                      _ptr(out), _mem(on_dev), _stream(stream, on_dev),
                                      ctypes.byref(n))
    L.check(rc, 'ctg_threshold_components')
    return out, int(n.value)


def merge_assignments(pairs, n_labels, stream=None, out=None):
    """ctg_merge_assignments: the union-find over the ids 0 .. n_labels - 1 with
    the (n, 2) ``pairs`` united -> (table, max_id): table[0] = 0, every other
    id maps to 1 + the rank of its set's smallest member (merge_assignments.py:
    125-132, the consecutive table).  ``pairs``: a numpy array (the table comes
    back as a uint64 array) or a contiguous 64-bit integer CUDA tensor (an int64
    tensor; ``out`` to write into an existing array of the same kind with
    n_labels 64-bit integers).  A pair member that is 0 or not below
    ``n_labels`` raises."""
    on_dev = _is_torch(pairs)
    if on_dev:
        if not (pairs.is_cuda and pairs.is_contiguous()) or pairs.element_size() != 8 or pairs.is_floating_point():
            raise ValueError('pairs must be a contiguous CUDA tensor of 64-bit integers')
    else:
        pairs = np.asarray(pairs)
        if pairs.size and pairs.dtype.kind not in 'ui':
            raise TypeError('pairs must hold integers, got %s' % pairs.dtype)
    if len(pairs.shape) != 2 or pairs.shape[1] != 2:
        raise ValueError('pairs must have shape (n, 2), got %s' % (tuple(pairs.shape),))
    if not 0 <= int(n_labels) < 1 << 64:
        raise ValueError('n_labels must be a uint64 value, got %r' % (n_labels,))
    n_labels = int(n_labels)
    if n_labels >= 1 << 32:
        raise ValueError('n_labels must stay below 2^32, got %d' % n_labels)
    table = _dense_out(out, (n_labels,), on_dev, pairs, 'int64', 'pairs', 'n_labels = %d entries' % n_labels)
    if not on_dev:
        if pairs.dtype.kind == 'i' and pairs.size and int(pairs.min()) < 0:
            raise ValueError('pairs holds negative values')
        pairs = np.ascontiguousarray(pairs, dtype=np.uint64)
    lib = L.load()
    L.init_device()
    max_id = ctypes.c_uint64(0)
    rc = lib.ctg_merge_assignments(_ptr(pairs), int(pairs.shape[0]), n_labels, _ptr(table),
                                   _mem(on_dev), _stream(stream, on_dev), ctypes.byref(max_id))
    L.check(rc, 'ctg_merge_assignments')
    return table, int(max_id.value)


EdtInfo = collections.namedtuple('EdtInfo', 'n_seeds n_unseeded argmax max_d2')


def _edt_source(src, threshold, label):
    """The source of a distance transform -> (array, CTG_EDT_SRC_*, bits)."""
    if threshold is not None and label is not None:
        raise ValueError('give a threshold (a float32 source) or a label (a label source), not both')
    on_dev = _is_torch(src)
    if on_dev:
        import torch
        if not (src.is_cuda and src.is_contiguous()):
            raise ValueError('src must be a contiguous CUDA tensor')
        kind = 'f' if src.dtype == torch.float32 else 'b' if src.dtype in (torch.uint8, torch.bool) else \
            'i' if not src.is_floating_point() and src.element_size() in (4, 8) else None
        if src.dtype == torch.bool:
            src = src.view(torch.uint8)
        bits = src.element_size() * 8
    else:
        src = np.asarray(src)
        kind = 'f' if src.dtype == np.float32 else 'b' if src.dtype in (np.uint8, np.bool_) else \
            'i' if src.dtype in (np.uint32, np.int32, np.uint64, np.int64) else None
        src = np.ascontiguousarray(src)
        if src.dtype == np.bool_:
            src = src.view(np.uint8)
        bits = src.dtype.itemsize * 8
    if label is not None:
        if kind != 'i':
            raise ValueError('a label needs a source of 32- or 64-bit integers, got %s' % src.dtype)
        if not 0 <= int(label) < 1 << 64:
            raise ValueError('label must be a uint64 value, got %r' % (label,))
        return src, L.CTG_EDT_SRC_EQUAL, bits
    if threshold is not None:
        if kind != 'f':
            raise ValueError('a threshold needs a float32 source, got %s (a label source takes label=)' % src.dtype)
        return src, L.CTG_EDT_SRC_GREATER, bits
    if kind != 'b':
        raise ValueError('a source without threshold or label must be uint8 or bool, got %s' % src.dtype)
    return src, L.CTG_EDT_SRC_NONZERO, bits


def _edt_pitch(pitch):
    if pitch is None:
        return None
    p = [float(v) for v in pitch]
    if len(p) != 3:
        raise ValueError('pitch must have 3 entries (z, y, x), got %d' % len(p))
    if not all(np.isfinite(v) and v > 0 for v in p):
        raise ValueError('every pitch must be finite and positive, got %r' % (tuple(p),))
    return p


def distance_transform(src, pitch=None, threshold=None, label=None, to_background=False, two_d=False, begin=None,
                       end=None, out=None, stream=None, squared=False):
    """ctg_distance_transform: the exact Euclidean distance transform of the
    box [begin, end) of ``src`` -> (dist, info).

    ``src``: a (Z,Y,X) numpy array or contiguous CUDA tensor.  The predicate P
    is ``x != 0`` for a uint8 / bool source, ``x > threshold`` (in float32; a
    NaN is not greater) for a float32 source with ``threshold``, ``x == label``
    for a 32- or 64-bit integer source with ``label``.  The seeds are the
    voxels where P holds -- vigra's distanceTransform(background=True): every
    other voxel's distance to the nearest of them -- or, with
    ``to_background``, those where it fails (scipy's distance_transform_edt).
    ``pitch``: the voxel size (z, y, x); ``two_d``: every z-slice on its own.
    ``dist``: box-shaped float32 (``out`` to write into an existing one),
    float32(sqrt(D2)) with D2 = (dz*pz)^2 + (dy*py)^2 + (dx*px)^2 in float64;
    a voxel whose box (slice, with ``two_d``) holds no seed gets that domain's
    diagonal.  With ``squared`` dist is float64 and holds D2 itself (the square
    of scipy's float64 result).  ``info``: (n_seeds, n_unseeded, argmax, max_d2) -- the seeds of
    the box, the voxels written with the diagonal, the flat index in the box of
    the first voxel with the largest D2, and that D2."""
    src, kind, bits = _edt_source(src, threshold, label)
    on_dev = _is_torch(src)
    shape = tuple(src.shape)
    if len(shape) != 3:
        raise ValueError('src must be 3-D, got shape %s' % (shape,))
    p = _edt_pitch(pitch)
    b, e, oshape = _box(shape, begin, end)
    out = _dense_out(out, oshape, on_dev, src, 'float64' if squared else 'float32', 'src')
    lib = L.load()
    L.init_device()
    info = (ctypes.c_uint64 * 4)()
    flags = (L.CTG_EDT_TO_BACKGROUND if to_background else 0) | (L.CTG_EDT_2D if two_d else 0) | \
        (L.CTG_EDT_OUT_D2 if squared else 0)
    rc = lib.ctg_distance_transform(_ptr(src), kind, bits, _shape_arr(shape), _shape_arr(b), _shape_arr(e),
                                    float(threshold or 0.0), int(label or 0),
                                    (ctypes.c_double * 3)(*p) if p is not None else None, flags, _ptr(out),
                                    _mem(on_dev), _stream(stream, on_dev), info)
    L.check(rc, 'ctg_distance_transform')
    return out, EdtInfo(int(info[0]), int(info[1]), int(info[2]),
                        float(np.array([info[3]], dtype=np.uint64).view(np.float64)[0]))


WsInfo = collections.namedtuple('WsInfo', 'max_id n_zero rounds n_dropped')
WS_MAX_VOXELS = 1 << 30


def seeded_watershed(hmap, seeds, size_filter=0, two_d=False, begin=None, end=None, out=None, stream=None):
    """ctg_seeded_watershed: the seeded watershed of the box [begin, end) of
    ``hmap`` -> (labels, info).

    ``hmap``: a (Z,Y,X) float32 numpy array or contiguous CUDA tensor; +-inf
    are ordinary heights, a NaN in the box raises and writes nothing.
    ``seeds``: of the same shape and kind, 32- or 64-bit integers, 0 = no seed.
    The result is the minimum spanning forest of the box's 6-neighbour graph
    (``two_d``: of every z-slice on its own) under the edge order of
    include/ctg.h, the seeded voxels contracted into one root: every voxel gets
    the label of the seed its tree hangs from, a label of minimal pass height;
    a voxel whose domain holds no seed stays 0.  ``size_filter``: labels with
    fewer voxels in a domain become 0 and the flood runs again from the
    survivors (elf's apply_size_filter).  ``labels``: box-shaped uint64 (an
    int64 tensor for tensors).  ``out`` writes into an existing one; it may be
    ``seeds`` itself where they are 64-bit and the box is the whole array.
    ``info``: (max_id, n_zero, rounds, n_dropped) -- the largest label written,
    the voxels left 0, the rounds of the last flood, the labels dropped."""
    on_dev = _is_torch(hmap)
    if _is_torch(seeds) != on_dev:
        raise ValueError('hmap and seeds must both be numpy arrays or both CUDA tensors')
    if on_dev:
        import torch
        if not (hmap.is_cuda and hmap.is_contiguous()) or hmap.dtype != torch.float32:
            raise ValueError('hmap must be a contiguous float32 CUDA tensor')
        if not (seeds.is_cuda and seeds.is_contiguous()) or seeds.is_floating_point() or \
                seeds.dtype == torch.bool or seeds.element_size() not in (4, 8):
            raise ValueError('seeds must be a contiguous CUDA tensor of 32- or 64-bit integers')
        bits = seeds.element_size() * 8
    else:
        hmap = np.asarray(hmap)
        seeds = np.asarray(seeds)
        if hmap.dtype != np.float32:
            raise TypeError('hmap must be float32, got %s' % hmap.dtype)
        if seeds.dtype not in (np.uint32, np.int32, np.uint64, np.int64):
            raise TypeError('seeds must be 32- or 64-bit integers, got %s' % seeds.dtype)
        bits = seeds.dtype.itemsize * 8
    shape = tuple(hmap.shape)
    if len(shape) != 3:
        raise ValueError('hmap must be 3-D, got shape %s' % (shape,))
    if tuple(seeds.shape) != shape:
        raise ValueError('seeds shape %s != hmap shape %s' % (tuple(seeds.shape), shape))
    if not 0 <= int(size_filter) < 1 << 64:
        raise ValueError('size_filter must be a uint64 value, got %r' % (size_filter,))
    b, e, oshape = _box(shape, begin, end)
    if oshape[0] * oshape[1] * oshape[2] > WS_MAX_VOXELS:
        raise ValueError('a box holds at most 2^30 voxels, got %s' % (oshape,))
    in_place = out is seeds
    if in_place and (bits != 64 or oshape != shape):
        raise ValueError('out may be the seeds only where they are 64-bit and the box is the whole array')
    if not on_dev:
        if np.isnan(hmap[b[0]:e[0], b[1]:e[1], b[2]:e[2]]).any():
            raise ValueError('the heights of the box hold a NaN')
        hmap = np.ascontiguousarray(hmap)
        if in_place and not seeds.flags.c_contiguous:
            raise ValueError('seeds written in place must be contiguous')
        seeds = np.ascontiguousarray(seeds)
        if in_place:
            out = seeds
    out = _dense_out(out, oshape, on_dev, hmap, 'int64', 'hmap')
    lib = L.load()
    L.init_device()
    info = (ctypes.c_uint64 * 4)()
    rc = lib.ctg_seeded_watershed(_ptr(hmap), _ptr(seeds), bits, _shape_arr(shape), _shape_arr(b), _shape_arr(e),
                                  L.CTG_WS_2D if two_d else 0, int(size_filter), _ptr(out),
                                  _mem(on_dev), _stream(stream, on_dev), info)
    L.check(rc, 'ctg_seeded_watershed')
    return out, WsInfo(int(info[0]), int(info[1]), int(info[2]), int(info[3]))


def synth_volume(shape, cell=10, seed=0, z_offset=0, global_shape=None, label_offset=0, noise_amp=0.1,
                 with_boundary=True, device=None):
    """Generate the synthetic volume directly in HBM (torch tensors)."""
    import torch
    lib = L.load()
    dev = L.init_device(device)
    labels = torch.empty(tuple(shape), dtype=torch.int64, device='cuda:%d' % dev)
    bnd = torch.empty(tuple(shape), dtype=torch.float32, device='cuda:%d' % dev) if with_boundary else None
    rc = lib.ctg_synth_volume(_ptr(labels), _ptr(bnd), _shape_arr(shape), int(z_offset), _shape_arr(global_shape),
                              int(cell), int(seed), int(label_offset), float(noise_amp),
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    L.check(rc, 'ctg_synth_volume')
    return labels, bnd


def synth_affinities(boundary, offsets):
    import torch
    lib = L.load()
    off = _check_offsets(offsets)
    shape = tuple(boundary.shape)
    affs = torch.empty((off.shape[0],) + shape, dtype=torch.float32, device=boundary.device)
    rc = lib.ctg_synth_affinities(_ptr(boundary), _ptr(affs), _shape_arr(shape), off.shape[0],
                                  off.ctypes.data_as(ctypes.c_void_p),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    L.check(rc, 'ctg_synth_affinities')
    return affs


def trim_cache():
    """Return the library's cached device memory (workspace + pool) to HIP."""
    L.init_device()
    L.check(L.load().ctg_trim(), 'ctg_trim')


def set_profiling(on=True):
    L.check(L.load().ctg_set_profiling(int(bool(on))), 'ctg_set_profiling')


def last_timings():
    """Device ms of the last rag call: scan, pack, sort, segment, reduce, nodes, total, and narrow (the
    uint64 -> u32 label pass of long-range affinity calls, before the scan; 0 when it did not run)."""
    buf = (ctypes.c_double * 8)()
    L.check(L.load().ctg_last_timings(buf, 8), 'ctg_last_timings')
    return dict(zip(['scan', 'pack', 'sort', 'segment', 'reduce', 'nodes', 'total', 'narrow'], list(buf)))


SORT_PATHS = ('bucket_keys', 'onesweep_keys', 'bucket_pairs', 'onesweep_pairs_wide', 'onesweep_pairs_default',
              'group')
SORT_DECLINES = ('none', 'n_range', 'key_bits', 'item_bits', 'low_bits', 'bucket_cap')


def last_sort():
    """Which way the last record sort of the current device went (ctg_last_sort, include/ctg.h): path (one
    of SORT_PATHS, None when there was no record), packed, group_tried, group_done, group_decline (one of
    SORT_DECLINES), group_shift, group_buckets, largest_bucket (-1: not read), ib, nb, ub and n."""
    buf = (ctypes.c_int64 * L.CTG_SORT_WORDS)()
    L.check(L.load().ctg_last_sort(buf, L.CTG_SORT_WORDS), 'ctg_last_sort')
    v = list(buf)
    return dict(path=SORT_PATHS[v[0]] if v[0] >= 0 else None, packed=v[1], group_tried=v[2], group_done=v[3],
                group_decline=SORT_DECLINES[v[4]], group_shift=v[5], group_buckets=v[6], largest_bucket=v[7],
                ib=v[8], nb=v[9], ub=v[10], n=v[11])


def last_scan():
    """Which plane loop the waves of the last whole-array face scan of the current device took
    (ctg_last_scan, include/ctg.h): waves and interior_waves of the launch of wide tiles, narrow_waves and
    narrow_interior_waves of the launch of narrow tiles (0: no such launch)."""
    buf = (ctypes.c_int64 * L.CTG_SCAN_WORDS)()
    L.check(L.load().ctg_last_scan(buf, L.CTG_SCAN_WORDS), 'ctg_last_scan')
    return dict(zip(['waves', 'interior_waves', 'narrow_waves', 'narrow_interior_waves'], list(buf)))
