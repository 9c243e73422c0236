"""Device time of ctg_region_features on a synthetic volume resident in HBM.

    python tools/region_features_timing.py [--sizes 512 1024] [--reps 5] [--rounds 3] [--overlaps] [--u8]

Labels: Voronoi supervoxels of cell 10, uint64; data: the synthetic boundary
map of the same volume, float32 (--u8: quantised to uint8) -- both generated on
the device.  Per size and round one JSON line: the library's HIP-event phase
times (ctg_last_timings: scan, sort, run heads + prefix sums, folds, total;
median of --reps calls after one warm-up), records per label, direct records,
and the scan's rate over its algorithmic bytes (12 B per voxel: an 8-byte label
and a 4-byte sample) as a fraction of 8 TB/s.  --overlaps adds, in the same
process, on the same label volume and in the same round, the scan time of
ctg_label_overlaps (values: a second labelling of cell 40, as
tools/overlap_timing.py; 16 B per voxel): the yardstick the region scan is read
against.
"""
import argparse
import json
import os
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
        rows.append((rag.last_timings(), r.info(), r.n_nodes))
        r.free()
    rows = rows[1:]
    return {k: float(np.median([x[0][k] for x in rows])) for k in PHASES}, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--overlaps', action='store_true')
    ap.add_argument('--u8', action='store_true')
    ap.add_argument('--ignore', type=int, default=None, help='ignore label (the HOLES instantiation)')
    args = ap.parse_args()
    import torch
    rag.set_profiling(True)
    for n in args.sizes:
        shape = (n, n, n)
        labels, data = rag.synth_volume(shape, cell=10, seed=1)
        if args.u8:
            data = (data.clamp(0, 1) * 255).to(torch.uint8)
        values = rag.synth_volume(shape, cell=40, seed=2, with_boundary=False)[0] if args.overlaps else None
        torch.cuda.synchronize()
        voxels = n ** 3
        bytes_per_voxel = 9.0 if args.u8 else 12.0
        for rnd in range(args.rounds):
            med, rows = median_phases(lambda: rag.region_features_handle(labels, data, ignore_label=args.ignore),
                                      args.reps)
            _, (n_rec, n_direct), n_labels = rows[-1]
            out = dict(size=n, round=rnd, voxels=voxels, reps=args.reps, data='u8' if args.u8 else 'f32',
                       ignore=args.ignore, lib=os.environ.get('CTG_LIB', ''), scan_ms=med['scan'],
                       sort_ms=med['sort'], heads_scan_ms=med['segment'], folds_ms=med['reduce'],
                       back_half_ms=med['total'] - med['scan'], total_ms=med['total'], records=n_rec,
                       direct=n_direct, labels=n_labels, records_per_label=n_rec / max(n_labels, 1),
                       scan_fraction_of_8TBs=bytes_per_voxel * voxels / (med['scan'] * 1e-3) / HBM_BYTES_PER_S,
                       scan_ms_all=[x[0]['scan'] for x in rows], total_ms_all=[x[0]['total'] for x in rows])
            if args.overlaps:
                omed, orows = median_phases(lambda: rag.label_overlaps_handle(labels, values), args.reps)
                out.update(overlap_scan_ms=omed['scan'], overlap_total_ms=omed['total'],
                           overlap_scan_fraction_of_8TBs=16.0 * voxels / (omed['scan'] * 1e-3) / HBM_BYTES_PER_S,
                           overlap_scan_ms_all=[x[0]['scan'] for x in orows],
                           region_over_overlap_scan=med['scan'] / omed['scan'])
            print(json.dumps(out), flush=True)
        del labels, data, values
        rag.trim_cache()


if __name__ == '__main__':
    main()
