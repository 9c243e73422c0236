"""Shared by the chunk-loop cases of test_overlaps_host, test_morphology_host and
test_region_features_host: a stand-in for a rag.Result with canned tables, and a
block dataset with a 1 x 1 x 3 chunk grid -- one chunk never written, one with
rows only outside [BEGIN, END), one with rows on both sides of each bound."""
import numpy as np

from cluster_tools_amd import n5

BEGIN, END = 4, 8
OUTSIDE_IDS = [1, 3, 8, 11]                 # the chunk at (0, 0, 1): END itself among them
MIXED_IDS = [2, 3, 4, 5, 7, 8, 9, 6]        # the chunk at (0, 0, 2): BEGIN - 1, BEGIN, END - 1, END; 6 out of order
IN_RANGE = [4, 5, 7, 6]                     # what a merge of [BEGIN, END) gets, in chunk order
N_OUT = 12                                  # rows of an output dataset


class Handle:
    """What a creating call of rag hands back, with canned tables: ``n_edges`` / ``n_nodes``, any accessor by
    its name, and free() -- by hand or at the end of a ``with`` -- counted."""

    def __init__(self, n_edges=0, n_nodes=0, **tables):
        self.n_edges, self.n_nodes, self.tables, self.freed = n_edges, n_nodes, tables, 0

    def __getattr__(self, name):
        if name in self.__dict__.get('tables', ()):
            return lambda *a, **kw: self.tables[name]
        raise AttributeError(name)

    def free(self):
        self.freed += 1

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def block_dataset(path, key, dtype, words_of):
    """The dataset of the docstring; ``words_of(ids)``: the chunk words of rows with those ids."""
    with n5.file_reader(path) as f:
        ds = f.require_dataset(key, shape=(1, 1, 3), chunks=(1, 1, 1), dtype=dtype, compression='gzip')
        ds.write_chunk((0, 0, 1), words_of(OUTSIDE_IDS), True)
        ds.write_chunk((0, 0, 2), words_of(MIXED_IDS), True)


def output_dataset(path, key, shape, dtype, chunks=None):
    with n5.file_reader(path) as f:
        f.require_dataset(key, shape=shape, chunks=chunks or shape, dtype=dtype, compression='gzip')


def read_output(path, key):
    with n5.file_reader(path, 'r') as f:
        return f[key][:]


def chunk_of(path, key, pos):
    with n5.file_reader(path, 'r') as f:
        return f[key].read_chunk(pos)


def capture(monkeypatch, module, name, result):
    """``module.name`` replaced by a function that records its arguments and returns ``result`` -> the record."""
    calls = []

    def fn(*a, **kw):
        calls.append((a, kw))
        return result
    monkeypatch.setattr(module, name, fn)
    return calls
