"""Device time of ctg_apply_assignment on a synthetic label volume resident in HBM.

    python tools/write_timing.py [--sizes 512 1024] [--reps 5] [--rounds 3] [--out profiles/write/timing.jsonl]

Labels: Voronoi supervoxels of cell 10, uint64, generated on the device.  The
assignment merges seeded groups of about eight labels: (a) as a dense table,
(b) the same mapping as a sparse table, (c) the dense table check-only (nothing
written).  Per size and round one JSON line: the library's HIP-event time of
the kernel (ctg_last_timings; median of --reps calls after one warm-up, and
every single call), its rate over the algorithmic bytes (16 B per voxel, 8
check-only) as a fraction of 8 TB/s, and the yardstick: a device-to-device copy
of the same label volume (out.copy_(labels), which also moves 8 + 8 B per
voxel), timed by HIP events on the same stream, in the same process and round,
with its own spread (largest - smallest single call).  The lines are appended to
--out as they are printed.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])

from cluster_tools_amd import rag  # noqa: E402

HBM_BYTES_PER_S = 8e12


def kernel_ms(call, reps):
    """The kernel times of ``reps`` calls after one warm-up."""
    ms = []
    for _ in range(reps + 1):
        call()
        ms.append(rag.last_timings()['scan'])
    return ms[1:]


def copy_ms(dst, src, reps):
    import torch
    ms = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default='profiles/write/timing.jsonl')
    args = ap.parse_args()
    import torch
    rag.set_profiling(True)
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    for n in args.sizes:
        labels = rag.synth_volume((n, n, n), cell=10, seed=1, with_boundary=False)[0]
        out = torch.empty_like(labels)
        n_labels = int(labels.max().item()) + 1
        table = np.random.default_rng(7).integers(1, max(2, n_labels // 8), size=n_labels).astype(np.uint64)
        table[0] = 0
        dense = rag.assignment_dense(table)
        sparse = rag.assignment_sparse(np.arange(n_labels, dtype=np.uint64), table)
        torch.cuda.synchronize()
        voxels = n ** 3
        for rnd in range(args.rounds):
            cp = copy_ms(out, labels, args.reps)
            d = kernel_ms(lambda: rag.apply_assignment(dense, labels, out=out), args.reps)
            s = kernel_ms(lambda: rag.apply_assignment(sparse, labels, out=out), args.reps)
            c = kernel_ms(lambda: rag.apply_assignment(dense, labels, check_only=True), args.reps)
            md, ms_, mc, mcp = (float(np.median(x)) for x in (d, s, c, cp))
            line = dict(size=n, round=rnd, voxels=voxels, reps=args.reps, labels=n_labels,
                        table_bytes_over_volume_bytes=n_labels / voxels, lib=os.environ.get('CTG_LIB', ''),
                        dense_ms=md, sparse_ms=ms_, check_only_ms=mc, copy_ms=mcp, copy_spread_ms=max(cp) - min(cp),
                        dense_within_copy_plus_spread=bool(md <= mcp + (max(cp) - min(cp))),
                        dense_over_copy=md / mcp, sparse_over_dense=ms_ / md,
                        dense_fraction_of_8TBs=16.0 * voxels / (md * 1e-3) / HBM_BYTES_PER_S,
                        sparse_fraction_of_8TBs=16.0 * voxels / (ms_ * 1e-3) / HBM_BYTES_PER_S,
                        check_only_fraction_of_8TBs=8.0 * voxels / (mc * 1e-3) / HBM_BYTES_PER_S,
                        copy_fraction_of_8TBs=16.0 * voxels / (mcp * 1e-3) / HBM_BYTES_PER_S,
                        dense_ms_all=d, sparse_ms_all=s, check_only_ms_all=c, copy_ms_all=cp)
            text = json.dumps(line)
            print(text, flush=True)
            with open(args.out, 'a') as f:
                f.write(text + '\n')
        dense.free()
        sparse.free()
        del labels, out
        rag.trim_cache()


if __name__ == '__main__':
    main()
