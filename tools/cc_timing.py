"""Device times of the thresholded components ("Thresholded
components"): rag.threshold_components on rag.synth_volume's boundary map at
threshold 0.5, per kernel (ctg_set_profiling / ctg_last_timings), and
rag.merge_assignments on random pairs.  One JSON line per measurement.

    python tools/cc_timing.py --sizes 256 512 --reps 5 --out profiles/thresholded_components/timing.jsonl
    python tools/cc_timing.py --scipy 256        # scipy.ndimage.label on the same map, on the CPU, one thread
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LABEL_PHASES = ('range', 'tiles', 'seams', 'flatten', 'scan', 'write', 'total')
MERGE_PHASES = ('init', 'pairs', 'flatten', 'scan', 'write', '-', 'total')
PEAK = 8e12   # bytes / s


def phases(names):
    from cluster_tools_amd import rag
    t = rag.last_timings()
    raw = [t[k] for k in ('scan', 'pack', 'sort', 'segment', 'reduce', 'nodes', 'total')]
    return {n: v for n, v in zip(names, raw) if n != '-'}


def median_phases(rows):
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='*', default=[512])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--labels', type=int, default=10 ** 7)
    ap.add_argument('--scipy', type=int, default=0)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    import torch
    from cluster_tools_amd import rag
    out = open(a.out, 'a') if a.out else sys.stdout

    def emit(rec):
        out.write(json.dumps(rec) + '\n')
        out.flush()

    rag.set_profiling(True)
    for size in a.sizes:
        _, bnd = rag.synth_volume((size,) * 3, cell=10, seed=0)
        V = size ** 3
        dst = torch.empty((size,) * 3, dtype=torch.int64, device=bnd.device)
        for c in (1, 3):
            for normalize in (True, False):
                rows, n = [], 0
                for rep in range(a.reps + 1):
                    _, n = rag.threshold_components(bnd, 0.5, connectivity=c, normalize=normalize, out=dst)
                    if rep:                      # the first call warms up
                        rows.append(phases(LABEL_PHASES))
                med = median_phases(rows)
                emit(dict(what='threshold_components', size=size, voxels=V, connectivity=c, normalize=normalize,
                          reps=a.reps, components=n, foreground=int((dst != 0).sum()), ms=med,
                          algorithmic_bytes=12 * V, fraction_of_8TBs=12 * V / (med['total'] * 1e-3) / PEAK,
                          total_ms_all=[r['total'] for r in rows]))
        del dst, bnd
    if a.labels:
        n_labels = a.labels
        g = torch.Generator(device='cuda').manual_seed(5)
        pairs = torch.randint(1, n_labels, (2 * n_labels, 2), dtype=torch.int64, device='cuda', generator=g)
        rows, max_id = [], 0
        for rep in range(a.reps + 1):
            _, max_id = rag.merge_assignments(pairs, n_labels)
            if rep:
                rows.append(phases(MERGE_PHASES))
        med = median_phases(rows)
        emit(dict(what='merge_assignments', n_labels=n_labels, pairs=int(pairs.shape[0]), reps=a.reps, max_id=max_id,
                  ms=med, total_ms_all=[r['total'] for r in rows]))
    if a.scipy:
        import scipy.ndimage as ndi
        size = a.scipy
        _, bnd = rag.synth_volume((size,) * 3, cell=10, seed=0)
        x = bnd.cpu().numpy()
        for c in (1, 3):
            structure = ndi.generate_binary_structure(3, c)
            t0 = time.perf_counter()
            v = x - x.min()
            v /= v.max()
            fg = v > np.float32(0.5)
            t1 = time.perf_counter()
            labels, n = ndi.label(fg, structure=structure)
            t2 = time.perf_counter()
            got, m = rag.threshold_components(bnd, 0.5, connectivity=c)
            same = bool(m == n and np.array_equal(got.cpu().numpy(), labels.astype(np.int64)))
            emit(dict(what='scipy.ndimage.label, one CPU thread', size=size, connectivity=c, components=int(n),
                      threshold_s=t1 - t0, label_s=t2 - t1, gpu_result_identical=same,
                      gpu_ms=phases(LABEL_PHASES)))


if __name__ == '__main__':
    main()
