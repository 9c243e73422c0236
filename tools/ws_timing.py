"""Device times of the seeded watershed ("Seeded watershed"):
rag.seeded_watershed on rag.synth_volume's boundary map, seeded by
rag.threshold_components of the map below a threshold, per phase
(ctg_set_profiling / ctg_last_timings; the phases are summed over the rounds).
One JSON line per measurement.

    python tools/ws_timing.py --shapes 512,512,512 50,512,512 --reps 3 --out profiles/watershed/timing.jsonl

Each shape runs plain, with size_filter 25 and in 2-D mode.  The line
`finished_sweep` floods the plain result again with one voxel unseeded: its two
rounds sweep over voxels that are all finished, which prices a round's pass
over finished voxels.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ('init', 'pick_hook', 'apply_chase', 'size_filter', 'write', '-', 'total')
PEAK = 8e12        # bytes / s
ALGO_BYTES = 20    # per voxel: 4 B of height + 8 B of seed + 8 B of label


def phases():
    from cluster_tools_amd import rag
    t = rag.last_timings()
    raw = [t[k] for k in ('scan', 'pack', 'sort', 'segment', 'reduce', 'nodes', 'total')]
    return {n: v for n, v in zip(PHASES, raw) if n != '-'}


def median_phases(rows):
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='*', default=['512,512,512', '50,512,512'])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--threshold', type=float, default=0.3)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    import torch
    from cluster_tools_amd import rag
    out = open(a.out, 'a') if a.out else sys.stdout

    def emit(rec):
        out.write(json.dumps(rec) + '\n')
        out.flush()

    rag.set_profiling(True)
    for text in a.shapes:
        shape = tuple(int(v) for v in text.split(','))
        V = int(np.prod(shape))
        _, bnd = rag.synth_volume(shape, cell=10, seed=0)
        seeds, n_seeds = rag.threshold_components(bnd, a.threshold, mode='less', connectivity=1)
        seed_ms = phases()['total']
        dst = torch.empty(shape, dtype=torch.int64, device=bnd.device)

        def measure(what, src, **kw):
            rows, info = [], None
            for rep in range(a.reps + 1):
                _, info = rag.seeded_watershed(bnd, src, out=dst, **kw)
                if rep:                      # the first call warms up
                    rows.append(phases())
            med = median_phases(rows)
            emit(dict(what=what, shape=shape, voxels=V, reps=a.reps, seeds=n_seeds,
                      seeded_voxels=int((src != 0).sum()), max_id=info.max_id, n_zero=info.n_zero,
                      rounds_last_flood=info.rounds, dropped=info.n_dropped, ms=med,
                      algorithmic_bytes=ALGO_BYTES * V,
                      achieved_bytes_per_s=ALGO_BYTES * V / (med['total'] * 1e-3),
                      fraction_of_8TBs=ALGO_BYTES * V / (med['total'] * 1e-3) / PEAK,
                      total_ms_all=[r['total'] for r in rows], threshold_components_ms=seed_ms))
            return med, info

        measure('seeded_watershed', seeds)
        again = dst.clone()
        again[shape[0] // 2, shape[1] // 2, shape[2] // 2] = 0
        med, info = measure('finished_sweep', again)
        emit(dict(what='finished_sweep_per_round', shape=shape,
                  ms_per_round=(med['pick_hook'] + med['apply_chase']) / max(info.rounds, 1)))
        del again
        measure('seeded_watershed size_filter=25', seeds, size_filter=25)
        measure('seeded_watershed two_d', seeds, two_d=True)
        del dst, bnd, seeds


if __name__ == '__main__':
    main()
