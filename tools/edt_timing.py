"""Device times of the exact Euclidean distance transform (DESIGN.md 5,
"Distance transform"): rag.distance_transform per pass (ctg_set_profiling /
ctg_last_timings) on rag.synth_volume's boundary map at threshold 0.5 (dense
seeds, short distances: the watershed's case) and on one object's EQUAL mask
in the whole label volume (few seeds, distances up to the box: the object
distances' case, the deepest envelope stacks), 3-D and 2-D, with and without a
pitch; and both stack placements at the line length where the plan switches.
Device-resident input and output, medians of --reps calls after a warm-up.
One JSON line per measurement.

    python tools/edt_timing.py --sizes 256 512 --reps 5 --out profiles/distance_transform/timing.jsonl
    python tools/edt_timing.py --sizes --scipy 256   # scipy's transform on the same map, on the CPU, one thread
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ('x', 'y', 'z', '-', '-', '-', 'total')
PEAK = 8e12   # bytes / s
LDS_LINE = 32   # csrc/ctg_plan.h: EDT_LDS_LINE


def phases():
    from cluster_tools_amd import rag
    t = rag.last_timings()
    raw = [t[k] for k in ('scan', 'pack', 'sort', 'segment', 'reduce', 'nodes', 'total')]
    return {n: v for n, v in zip(PHASES, raw) if n != '-'}


def measure(emit, reps, what, src, src_bytes, **kw):
    import torch
    from cluster_tools_amd import rag
    shape = tuple(src.shape)
    V = int(np.prod(shape))
    dst = torch.empty(shape, dtype=torch.float32, device=src.device)
    rows, info = [], None
    for rep in range(reps + 1):
        _, info = rag.distance_transform(src, out=dst, **kw)
        if rep:                                  # the first call warms up
            rows.append(phases())
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    two_d = bool(kw.get('two_d'))
    design = (src_bytes + (8 if two_d or shape[0] == 1 else 16)) * V      # s + 2 | 2 + 4 | 4 + 4 (2-D: no z pass)
    algorithmic = (src_bytes + 4) * V
    sec = med['total'] * 1e-3
    emit(dict(what=what, shape=shape, voxels=V, two_d=two_d, pitch=kw.get('pitch'), reps=reps, ms=med,
              total_ms_min_max=[min(r['total'] for r in rows), max(r['total'] for r in rows)],
              seeds=info.n_seeds, unseeded=info.n_unseeded, max_distance=float(np.sqrt(info.max_d2)),
              design_bytes=design, design_fraction_of_8TBs=design / sec / PEAK,
              algorithmic_bytes=algorithmic, algorithmic_fraction_of_8TBs=algorithmic / sec / PEAK))
    return dst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='*', default=[256])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--switch', type=int, default=0, help='y, x extent of the boxes at the plan switch (0: skip)')
    ap.add_argument('--scipy', type=int, default=0)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library opens the device, as tools/cc_timing.py)
    from cluster_tools_amd import rag
    out = open(a.out, 'a') if a.out else sys.stdout

    def emit(rec):
        out.write(json.dumps(rec) + '\n')
        out.flush()

    rag.set_profiling(True)
    for size in a.sizes:
        lab, bnd = rag.synth_volume((size,) * 3, cell=10, seed=0)
        one = int(lab[size // 2, size // 2, size // 2])
        for two_d in (False, True):
            for pitch in (None,) if two_d else (None, (40, 4, 4)):
                measure(emit, a.reps, 'boundary > 0.5', bnd, 4, threshold=0.5, two_d=two_d, pitch=pitch)
                measure(emit, a.reps, 'one object, EQUAL', lab, 8, label=one, two_d=two_d, pitch=pitch)
        del lab, bnd
    if a.switch:
        # the z line at the LDS limit and one past it: the same work per voxel, the stacks in LDS / in the buffer
        for nz in (LDS_LINE, LDS_LINE + 1):
            lab, bnd = rag.synth_volume((nz, a.switch, a.switch), cell=10, seed=0)
            one = int(lab[nz // 2, a.switch // 2, a.switch // 2])
            measure(emit, a.reps, 'plan switch, boundary > 0.5', bnd, 4, threshold=0.5)
            measure(emit, a.reps, 'plan switch, one object, EQUAL', lab, 8, label=one)
            del lab, bnd
    if a.scipy:
        import scipy.ndimage as ndi
        size = a.scipy
        _, bnd = rag.synth_volume((size,) * 3, cell=10, seed=0)
        x = bnd.cpu().numpy()
        for pitch in (None, (40, 4, 4)):
            t0 = time.perf_counter()
            want = ndi.distance_transform_edt(~(x > np.float32(0.5)), sampling=pitch)
            t1 = time.perf_counter()
            got, _ = rag.distance_transform(bnd, threshold=0.5, pitch=pitch)
            same = bool(np.array_equal(got.cpu().numpy(), want.astype(np.float32)))
            emit(dict(what='scipy.ndimage.distance_transform_edt, one CPU thread', size=size, pitch=pitch,
                      scipy_s=t1 - t0, gpu_result_identical=same, gpu_ms=phases()))


if __name__ == '__main__':
    main()
