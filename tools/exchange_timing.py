"""Wall time of ctg_mgpu_pack and ctg_mgpu_merge at world > 1 on ONE device
("Exchange host layer"): tests/exchange_sim.simulate runs every
rank's exchange steps of the synthetic volume in this process, with written
statistics rows (HipBackend(defer_stats=False)) and with deferred ones
(defer_stats=True, every rank's local call re-run before its pack and merge).
Every pack and merge is timed with a stream synchronise before and after the
call; a run's pack_ms / merge_ms is the sum over the ranks, and the line
reports the median over --reps runs after one warm-up, and every run.

    CTG_LIB=variants/libctg_parent.so python tools/exchange_timing.py --out profiles/exchange_refactor/timing.jsonl
    python tools/exchange_timing.py --round 0 --out profiles/exchange_refactor/timing.jsonl

The ranks share the device, so the figures compare two builds of the library;
they are no projection of a multi-GPU step.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--world', type=int, default=4)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--round', type=int, default=0)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    import torch
    from cluster_tools_amd import dist as cdist
    from cluster_tools_amd import rag
    from tests.exchange_sim import simulate

    class Timed(cdist.HipBackend):
        """HipBackend whose pack and merge note their synchronised wall time."""
        ms = None

        def _timed(self, key, call, *args):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = call(*args)
            torch.cuda.synchronize()
            self.ms[key] += (time.perf_counter() - t0) * 1e3
            return out

        def pack(self, *args):
            return self._timed('pack', super().pack, *args)

        def merge(self, *args):
            return self._timed('merge', super().merge, *args)

    lab, bnd = rag.synth_volume((a.size,) * 3, cell=10, seed=0)
    for defer in (False, True):
        backend = Timed(defer_stats=defer)
        runs, rows = [], 0
        for rep in range(a.reps + 1):
            backend.ms = dict(pack=0.0, merge=0.0)
            shards = simulate(backend, lab, bnd, a.world, fresh=defer)
            rows = sum(int(x.n_edges) for x in shards)
            for x in shards:
                x.free()
            if rep:                                  # the first run warms up
                runs.append(backend.ms)
        line = dict(what='exchange_sim', lib=os.environ.get('CTG_LIB', ''), round=a.round, size=a.size, world=a.world,
                    defer_stats=defer, reps=a.reps, edges=rows,
                    pack_ms=float(np.median([r['pack'] for r in runs])),
                    merge_ms=float(np.median([r['merge'] for r in runs])),
                    pack_ms_all=[r['pack'] for r in runs], merge_ms_all=[r['merge'] for r in runs])
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(text + '\n')


if __name__ == '__main__':
    main()
