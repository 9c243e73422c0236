"""Host time of the small label-table calls, where the Python layer is most of the cost.

    python tools/table_call_timing.py [--package DIR] [--calls 1000] [--tag NAME]

1 x 1 x 2 numpy volumes and 2-row tables through the package under DIR (default: this tree; CTG_LIB picks the
library, so two Python layers can be timed over one binary).  One JSON line per row: the wall time per call of a
loop of --calls calls (``us``), and -- from a second loop in which every library function is timed from Python --
the part of it spent outside the library (``python_share``).  Rows: the host conveniences label_overlaps,
morphology, region_features; the dense readers max_overlaps, morphology_rows, region_feature_rows of tables; and
every host accessor of a Result on a handle of such a call.
"""
import argparse
import json
import os
import sys
import time

import numpy as np


class Timed:
    """The library with every function call timed."""

    def __init__(self, lib):
        self.lib, self.spent = lib, 0.0

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(*args):
            t = time.perf_counter()
            try:
                return fn(*args)
            finally:
                self.spent += time.perf_counter() - t
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--package', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--calls', type=int, default=1000)
    ap.add_argument('--tag', default='tree')
    args = ap.parse_args()
    sys.path.insert(0, args.package)
    from cluster_tools_amd import _lib, rag

    lab = np.array([[[1, 2]]], np.uint64)
    val = np.array([[[3, 3]]], np.uint64)
    dat = np.array([[[0.25, 0.5]]], np.float32)
    pairs, counts = np.array([[1, 3], [2, 3]], np.uint64), np.array([1, 1], np.uint64)
    morph = rag.morphology(lab)['rows']
    region = rag.region_features(lab, dat)['rows']
    handles = dict(overlaps=rag.label_overlaps_handle(lab, val), morphology=rag.morphology_handle(lab),
                   region=rag.region_features_handle(lab, dat), rag=rag.rag_features_handle(lab, dat, keep_stats=True))
    rows = {
        'label_overlaps': lambda: rag.label_overlaps(lab, val),
        'morphology': lambda: rag.morphology(lab),
        'region_features': lambda: rag.region_features(lab, dat),
        'max_overlaps': lambda: rag.max_overlaps(dict(pairs=pairs, counts=counts), 0, 4),
        'morphology_rows': lambda: rag.morphology_rows(dict(rows=morph), 0, 4),
        'region_feature_rows': lambda: rag.region_feature_rows(dict(rows=region), 0, 4),
        'Result.edges': handles['rag'].edges, 'Result.nodes': handles['rag'].nodes,
        'Result.features': handles['rag'].features, 'Result.stats': handles['rag'].stats,
        'Result.counts': handles['overlaps'].counts, 'Result.moments': handles['morphology'].moments,
        'Result.morph_rows': handles['morphology'].morph_rows,
        'Result.region_moments': handles['region'].region_moments,
        'Result.region_rows': handles['region'].region_rows,
    }
    real_load = _lib.load
    for name, call in rows.items():
        for _ in range(20):
            call()
        t = time.perf_counter()
        for _ in range(args.calls):
            call()
        wall = (time.perf_counter() - t) / args.calls
        timed = Timed(real_load())
        _lib.load = lambda: timed
        try:
            t = time.perf_counter()
            for _ in range(args.calls):
                call()
            wall_timed = time.perf_counter() - t
        finally:
            _lib.load = real_load
        print(json.dumps(dict(tool='table_calls', tag=args.tag, row=name, calls=args.calls, us=wall * 1e6,
                              python_share=1.0 - timed.spent / wall_timed)), flush=True)
    for h in handles.values():
        h.free()


if __name__ == '__main__':
    main()
