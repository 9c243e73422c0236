"""The argument errors of the assignment entry points of the C ABI
(ctg_assignment_dense / _sparse / _info / _free, ctg_apply_assignment) that are
decided before any GPU work: status and message of every such return, called
through the built library with small numpy buffers (no GPU: each call returns
at its argument checks).  Where two errors apply at once the case pins which one
is reported.  A failing call leaves *out null."""
import ctypes

import numpy as np
import pytest

from cluster_tools_amd import _lib

ARG, UNSUPPORTED = -1, -4
SENTINEL = 0xDEAD0


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def fails(lib, rc, status, text, out=None):
    msg = lib.ctg_last_error().decode()
    assert rc == status, (rc, msg)
    assert text in msg, msg
    if out is not None:
        assert not out.value, 'a failing call left *out set'


TABLE = np.arange(8, dtype=np.uint64)


@pytest.mark.parametrize('kw,text', [
    (dict(out=False), 'ctg_assignment_dense: bad arguments'),
    (dict(n=-1), 'ctg_assignment_dense: bad arguments'),
    (dict(table=None), 'ctg_assignment_dense: bad arguments'),
    (dict(mem=7), 'ctg_assignment_dense: mem must be'),
    (dict(n=-1, mem=7), 'bad arguments'),
])
def test_assignment_dense_errors(lib, kw, text):
    a = dict(table=TABLE, n=8, mem=_lib.CTG_MEM_HOST, out=True)
    a.update(kw)
    o = ctypes.c_void_p(SENTINEL)
    rc = lib.ctg_assignment_dense(ptr(a['table']), a['n'], a['mem'], None, ctypes.byref(o) if a['out'] else None)
    fails(lib, rc, ARG, text, o if a['out'] else None)


@pytest.mark.parametrize('kw,status,text', [
    (dict(out=False), ARG, 'ctg_assignment_sparse: bad arguments'),
    (dict(n=-1), ARG, 'ctg_assignment_sparse: bad arguments'),
    (dict(keys=None), ARG, 'ctg_assignment_sparse: bad arguments'),
    (dict(values=None), ARG, 'ctg_assignment_sparse: bad arguments'),
    (dict(mem=-1), ARG, 'ctg_assignment_sparse: mem must be'),
    (dict(n=(1 << 40) + 1), UNSUPPORTED, 'more than 2^40 pairs'),
    (dict(n=(1 << 40) + 1, mem=3), ARG, 'mem must be'),
])
def test_assignment_sparse_errors(lib, kw, status, text):
    a = dict(keys=TABLE, values=TABLE, n=8, mem=_lib.CTG_MEM_HOST, out=True)
    a.update(kw)
    o = ctypes.c_void_p(SENTINEL)
    rc = lib.ctg_assignment_sparse(ptr(a['keys']), ptr(a['values']), a['n'], a['mem'], None,
                                   ctypes.byref(o) if a['out'] else None)
    fails(lib, rc, status, text, o if a['out'] else None)


def test_assignment_info_and_free_of_null(lib):
    fails(lib, lib.ctg_assignment_info(None, None, None, None), ARG, 'ctg_assignment_info: null handle')
    lib.ctg_assignment_free(None)


class FakeAssignment(ctypes.Structure):
    """The head of ctg_assignment (csrc/ctg_internal.h) -- enough for the
    argument checks, which read its kind and never reach its table."""
    _fields_ = [('device', ctypes.c_int), ('kind', ctypes.c_int), ('n', ctypes.c_int64),
                ('max_value', ctypes.c_uint64), ('table', ctypes.c_void_p), ('size', ctypes.c_uint64)]


LABELS = np.zeros(16, dtype=np.uint64)
OUT = np.zeros(16, dtype=np.uint64)


def i64(*v):
    return np.array(v, dtype=np.int64)


def u64(*v):
    return np.array(v, dtype=np.uint64)


def odd(a, itemsize):
    """A view of ``a``'s buffer that starts ``itemsize`` / 2 bytes in: misaligned."""
    return np.frombuffer(a.tobytes() + b'\0' * 8, dtype=np.uint8)[itemsize // 2:]


APPLY_ERRORS = [
    (dict(a=False), ARG, 'ctg_apply_assignment: null argument'),
    (dict(labels=None), ARG, 'ctg_apply_assignment: null argument'),
    (dict(seg_nonzero=None), ARG, 'ctg_apply_assignment: null argument'),
    (dict(missing=None), ARG, 'ctg_apply_assignment: null argument'),
    (dict(seg_begin=i64(0, 16), n_seg=1), ARG, 'ctg_apply_assignment: null argument'),          # no seg_offset
    (dict(label_bits=16), ARG, 'label_bits must be 32 or 64'),
    (dict(mem=2), ARG, 'mem must be CTG_MEM_HOST or CTG_MEM_DEVICE'),
    (dict(n=-1), ARG, 'negative n or n_seg'),
    (dict(seg_begin=i64(0, 16), seg_offset=u64(0), n_seg=-1), ARG, 'negative n or n_seg'),
    (dict(seg_begin=i64(0, 16), seg_offset=u64(0), n_seg=1 << 31), UNSUPPORTED, '2^31 segments'),
    (dict(seg_begin=i64(1, 16), seg_offset=u64(0), n_seg=1), ARG, 'seg_begin must ascend from 0 to n'),
    (dict(seg_begin=i64(0, 15), seg_offset=u64(0), n_seg=1), ARG, 'seg_begin must ascend from 0 to n'),
    (dict(seg_begin=i64(0, 9, 8, 16), seg_offset=u64(0, 0, 0), n_seg=3), ARG, 'seg_begin must ascend from 0 to n'),
    (dict(seg_begin=i64(0), seg_offset=u64(), n_seg=0), ARG, 'seg_begin must ascend from 0 to n'),   # 16 voxels, no segment
    (dict(n=1 << 43), UNSUPPORTED, '2^43 voxels or more'),
    (dict(allow_missing=1), ARG, 'allow_missing needs a sparse assignment'),
    (dict(label_bits=32, out=LABELS), ARG, 'in place needs 64-bit labels'),
    (dict(labels=odd(LABELS, 8)), ARG, 'must be aligned'),
    (dict(label_bits=32, labels=odd(LABELS, 4)), ARG, 'must be aligned'),
    (dict(out=odd(OUT, 8)), ARG, 'must be aligned'),
    # two errors at once: the checks run in the order above
    (dict(labels=None, label_bits=16), ARG, 'null argument'),
    (dict(label_bits=16, n=-1), ARG, 'label_bits must be 32 or 64'),
    (dict(n=-1, allow_missing=1), ARG, 'negative n or n_seg'),
    (dict(seg_begin=i64(0, 15), seg_offset=u64(0), n_seg=1, allow_missing=1), ARG, 'seg_begin must ascend'),
    (dict(allow_missing=1, label_bits=32, out=LABELS), ARG, 'allow_missing needs'),
]


@pytest.mark.parametrize('kw,status,text', APPLY_ERRORS)
def test_apply_assignment_errors(lib, kw, status, text):
    fake = FakeAssignment(device=0, kind=_lib.CTG_ASSIGN_DENSE, n=8, max_value=7, table=None, size=8)
    a = dict(a=True, labels=LABELS, label_bits=64, n=16, seg_begin=None, seg_offset=None, n_seg=0, allow_missing=0,
             out=OUT, seg_nonzero=u64(0, 0, 0, 0), missing=u64(0, 0), mem=_lib.CTG_MEM_HOST)
    a.update(kw)
    rc = lib.ctg_apply_assignment(ctypes.byref(fake) if a['a'] else None, ptr(a['labels']), a['label_bits'], a['n'],
                                  ptr(a['seg_begin']), ptr(a['seg_offset']), a['n_seg'], a['allow_missing'],
                                  ptr(a['out']), ptr(a['seg_nonzero']), ptr(a['missing']), a['mem'], None)
    fails(lib, rc, status, text)


def test_allow_missing_is_fine_with_a_sparse_assignment(lib):
    """... so the same call with a sparse handle passes that check and is refused by the next one."""
    fake = FakeAssignment(device=0, kind=_lib.CTG_ASSIGN_SPARSE, n=8, max_value=7, table=None, size=64)
    rc = lib.ctg_apply_assignment(ctypes.byref(fake), ptr(LABELS), 32, 16, None, None, 0, 1, ptr(LABELS),
                                  ptr(u64(0)), ptr(u64(0, 0)), _lib.CTG_MEM_HOST, None)
    fails(lib, rc, ARG, 'in place needs 64-bit labels')


def test_python_layer_refuses_before_the_library():
    from cluster_tools_amd import rag
    with pytest.raises(TypeError, match='live Assignment'):
        rag.apply_assignment(None, LABELS)
    with pytest.raises(ValueError, match='1-D'):
        rag.assignment_dense(np.zeros((2, 2), dtype=np.uint64))
    with pytest.raises(TypeError, match='integers'):
        rag.assignment_dense(np.zeros(2, dtype=np.float64))
    with pytest.raises(ValueError, match='negative'):
        rag.assignment_sparse(np.array([1, -2]), np.array([1, 2]))
    with pytest.raises(ValueError, match='3 keys for 2 values'):
        rag.assignment_sparse(np.arange(3), np.arange(2))
