"""Device time of ctg_morphology on a synthetic label volume resident in HBM.

    python tools/morphology_timing.py [--sizes 512 1024] [--reps 5] [--overlaps]

Labels: Voronoi supervoxels of cell 10, uint64, generated on the device.  Per
size one JSON line: the library's HIP-event phase times (ctg_last_timings: scan,
sort, run heads + prefix sums, folds, total; median of --reps calls after one
warm-up), records per label, direct records, and the scan's rate over its
algorithmic bytes (8 B per voxel) as a fraction of 8 TB/s.  --overlaps adds, in
the same process and on the same label volume, the scan time of
ctg_label_overlaps (values: a second labelling of cell 40, as
tools/overlap_timing.py): the yardstick the morphology scan is read against.
"""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])

from cluster_tools_amd import rag  # noqa: E402

HBM_BYTES_PER_S = 8e12
PHASES = ('scan', 'sort', 'segment', 'reduce', 'total')


def median_phases(call, reps):
    """Median phase times of ``reps`` calls after one warm-up, and the last handle's counts."""
    rows = []
    for _ in range(reps + 1):
        r = call()
        rows.append((rag.last_timings(), r.info(), r.n_nodes, r.n_edges))
        r.free()
    rows = rows[1:]
    med = {k: float(np.median([x[0][k] for x in rows])) for k in PHASES}
    return med, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--overlaps', action='store_true')
    args = ap.parse_args()
    import torch
    rag.set_profiling(True)
    for n in args.sizes:
        shape = (n, n, n)
        labels, _ = rag.synth_volume(shape, cell=10, seed=1, with_boundary=False)
        torch.cuda.synchronize()
        med, rows = median_phases(lambda: rag.morphology_handle(labels), args.reps)
        _, (n_rec, n_direct), n_labels, _ = rows[-1]
        voxels = n ** 3
        out = dict(size=n, voxels=voxels, reps=args.reps, scan_ms=med['scan'], sort_ms=med['sort'],
                   heads_scan_ms=med['segment'], folds_ms=med['reduce'], back_half_ms=med['total'] - med['scan'],
                   total_ms=med['total'], records=n_rec, direct=n_direct, labels=n_labels,
                   records_per_label=n_rec / max(n_labels, 1),
                   scan_fraction_of_8TBs=8.0 * voxels / (med['scan'] * 1e-3) / HBM_BYTES_PER_S,
                   scan_ms_all=[x[0]['scan'] for x in rows], total_ms_all=[x[0]['total'] for x in rows])
        if args.overlaps:
            values, _ = rag.synth_volume(shape, cell=40, seed=2, with_boundary=False)
            torch.cuda.synchronize()
            omed, orows = median_phases(lambda: rag.label_overlaps_handle(labels, values), args.reps)
            out.update(overlap_scan_ms=omed['scan'], overlap_total_ms=omed['total'],
                       overlap_scan_fraction_of_8TBs=16.0 * voxels / (omed['scan'] * 1e-3) / HBM_BYTES_PER_S,
                       overlap_scan_ms_all=[x[0]['scan'] for x in orows],
                       morphology_over_overlap_scan=med['scan'] / omed['scan'])
            del values
        print(json.dumps(out), flush=True)
        del labels
        rag.trim_cache()


if __name__ == '__main__':
    main()
