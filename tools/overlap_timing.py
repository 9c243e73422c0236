"""Device time of ctg_label_overlaps on synthetic volumes resident in HBM.

    python tools/overlap_timing.py [--sizes 512 1024] [--reps 5] [--oracle-size 512]

Labels: Voronoi supervoxels of cell 10; values: a second labelling of cell 40
(both uint64, generated on the device).  Per size one JSON line: the library's
HIP-event phase times (ctg_last_timings: scan, sort, run heads + prefix sums,
run sums, total; median of --reps calls after one warm-up), records per unique
pair, and the scan's rate over its algorithmic bytes (16 B per voxel) as a
fraction of 8 TB/s.  --oracle-size N adds the numpy oracle's wall time
(np.unique of the stacked pairs, on the CPU) on the N^3 arrays.
"""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])

from cluster_tools_amd import rag  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--oracle-size', type=int, default=0)
    args = ap.parse_args()
    import torch
    rag.set_profiling(True)
    for n in args.sizes:
        shape = (n, n, n)
        labels, _ = rag.synth_volume(shape, cell=10, seed=1, with_boundary=False)
        values, _ = rag.synth_volume(shape, cell=40, seed=2, with_boundary=False)
        torch.cuda.synchronize()
        rows = []
        for rep in range(args.reps + 1):
            r = rag.label_overlaps_handle(labels, values)
            t = rag.last_timings()
            n_rec, n_direct = r.info()
            rows.append((t, n_rec, n_direct, r.n_edges, r.n_nodes))
            r.free()
        rows = rows[1:]
        med = {k: float(np.median([x[0][k] for x in rows])) for k in ('scan', 'sort', 'segment', 'reduce', 'total')}
        _, n_rec, n_direct, n_pairs, n_nodes = rows[-1]
        voxels = n ** 3
        out = dict(size=n, voxels=voxels, reps=args.reps, scan_ms=med['scan'], sort_ms=med['sort'],
                   heads_scan_ms=med['segment'], runs_ms=med['reduce'], sort_runs_ms=med['total'] - med['scan'],
                   total_ms=med['total'], records=n_rec, direct=n_direct, pairs=n_pairs, nodes=n_nodes,
                   records_per_pair=n_rec / max(n_pairs, 1),
                   scan_fraction_of_8TBs=16.0 * voxels / (med['scan'] * 1e-3) / HBM_BYTES_PER_S,
                   scan_ms_all=[x[0]['scan'] for x in rows], total_ms_all=[x[0]['total'] for x in rows])
        if n == args.oracle_size:
            a = labels.cpu().numpy().view(np.uint64).ravel()
            b = values.cpu().numpy().view(np.uint64).ravel()
            t0 = time.perf_counter()
            pairs, counts = np.unique(np.stack([a, b], 1), axis=0, return_counts=True)
            out['numpy_oracle_s'] = time.perf_counter() - t0
            out['numpy_pairs'] = int(pairs.shape[0])
            assert pairs.shape[0] == n_pairs and int(counts.sum()) == voxels
        print(json.dumps(out), flush=True)
        del labels, values
        rag.trim_cache()


if __name__ == '__main__':
    main()
