"""The host layer's decisions (csrc/ctg_plan.h: tile depths, record-sort path,
channel classes, bucket key range) are pure functions; tools/plan_check.cpp
drives them on the CPU -- built with the host compiler and
-fsanitize=address,undefined -- and its answers are compared with the tables
below (no GPU, no library)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROWS_WIDE, ROWS_NARROW = 32, 8    # CTG_ROWS 4 x 8 waves, CTG_ROWS_NARROW 1 x 8 (ctg_scan.hip)


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('plan') / 'plan_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', os.path.join(ROOT, 'tools', 'plan_check.cpp'), '-o', exe],
                   check=True, capture_output=True, timeout=300)

    def ask(queries):
        r = subprocess.run([exe], input='\n'.join(queries) + '\n', capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        out = r.stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return ask


def test_bits_for(plan):
    vals = [0, 1, 2, 3, 255, 256, (1 << 32) - 1, 1 << 32, (1 << 64) - 1]
    got = plan(['bits %d' % v for v in vals])
    assert [int(g) for g in got] == [max(1, v.bit_length()) for v in vals]


# (z, y, x) -> (tile_z, tile_z_narrow)
TILE_DEPTHS = [
    ((24, 40, 72), (8, 8)),
    ((128, 256, 256), (8, 8)),
    ((512, 512, 512), (32, 16)),
    ((640, 640, 640), (32, 16)),
    ((1024, 1024, 1024), (32, 32)),
    ((2048, 2048, 2048), (128, 128)),
    ((1025, 2048, 2048), (128, 128)),
    ((513, 2048, 2048), (128, 128)),
    ((257, 2048, 2048), (128, 64)),
    ((1, 2048, 2048), (32, 16)),
]


def test_tile_depths(plan):
    got = plan(['tile %d %d %d %d %d' % (s + (ROWS_WIDE, ROWS_NARROW)) for s, _ in TILE_DEPTHS])
    assert [tuple(map(int, g.split())) for g in got] == [t for _, t in TILE_DEPTHS]


def _sort(has_keys=1, has_regions=1, n=0, ub=0, nb=0, ib=0, spread=1, packed=1, bucket=1, bucket_pairs=-1,
          group=1, group_first=0):
    return 'sort %d %d %d %d %d %d %d %d %d %d %d %d' % (has_keys, has_regions, n, ub, nb, ib, spread, packed,
                                                         bucket, bucket_pairs, group, group_first)


# the scan-record cases: name -> (inputs, (packed, try_group, path))
SCAN_SORTS = {
    '512^3-like': (dict(n=1900000, ub=17, nb=17, ib=23), (1, 0, 'bucket_keys')),
    '2048^3-like': (dict(n=27800000, ub=22, nb=22, ib=29), (0, 1, 'bucket_pairs')),
    'configs[4]-like': (dict(n=110000000, ub=24, nb=24, ib=28), (0, 1, 'onesweep_pairs_default')),
    'tagged, fits': (dict(n=1000000, ub=32, nb=13, ib=18, spread=0), (1, 0, 'onesweep_keys')),
    'tagged, does not fit': (dict(n=1000000, ub=32, nb=14, ib=18, spread=0), (0, 0, 'onesweep_pairs_wide')),
}


def _answers(plan, queries):
    return [(int(p), int(g), path) for p, g, path in (a.split() for a in plan(queries))]


def test_record_sort_scan_cases(plan):
    got = _answers(plan, [_sort(**kw) for kw, _ in SCAN_SORTS.values()])
    assert got == [exp for _, exp in SCAN_SORTS.values()]
    # CTG_GROUP_FIRST=1: packable records are offered to the group sort, which may decline
    assert _answers(plan, [_sort(group_first=1, **SCAN_SORTS['512^3-like'][0])]) == [(1, 1, 'bucket_keys')]


def test_record_sort_pair_input(plan):
    got = _answers(plan, [_sort(has_keys=0, has_regions=0, n=1000, ub=10, nb=10),
                          _sort(has_keys=0, has_regions=0, n=1000, ub=10, nb=10, bucket_pairs=0),
                          # dense keys without regions (no slot to pack): pairs as well
                          _sort(has_keys=1, has_regions=0, n=1000, ub=10, nb=10)])
    assert got == [(0, 0, 'bucket_pairs'), (0, 0, 'onesweep_pairs_wide'), (0, 0, 'bucket_pairs')]


def test_record_sort_switches(plan):
    cases = list(SCAN_SORTS.values())
    off_packed = _answers(plan, [_sort(packed=0, **kw) for kw, _ in cases])
    off_group = _answers(plan, [_sort(group=0, **kw) for kw, _ in cases])
    off_bucket = _answers(plan, [_sort(bucket=0, **kw) for kw, _ in cases])
    for (kw, exp), p, g, b in zip(cases, off_packed, off_group, off_bucket):
        assert p[0] == 0
        assert g == (exp[0], 0, exp[2])
        assert b == (exp[0], exp[1], 'onesweep_keys' if exp[2] == 'bucket_keys' else exp[2])
    # CTG_BUCKET_SORT_PAIRS=1 forces the bucket pass past its record limit
    assert _answers(plan, [_sort(bucket_pairs=1, **SCAN_SORTS['configs[4]-like'][0])])[0][2] == 'bucket_pairs'


def test_record_sort_thresholds(plan):
    """63 key + slot bits pack, 64 do not; wide digits up to 64 Mi records, the
    pair path's bucket sort up to 32 Mi."""
    got = _answers(plan, [_sort(n=1000, ub=20, nb=20, ib=23), _sort(n=1000, ub=20, nb=20, ib=24),
                          _sort(n=64 << 20, ub=17, nb=17, ib=27), _sort(n=(64 << 20) + 1, ub=17, nb=17, ib=27),
                          _sort(n=32 << 20, ub=22, nb=22, ib=29), _sort(n=(32 << 20) + 1, ub=22, nb=22, ib=29),
                          _sort(n=(64 << 20) + 1, ub=22, nb=22, ib=29)])
    assert got == [(1, 0, 'bucket_keys'), (0, 1, 'bucket_pairs'),
                   (1, 0, 'bucket_keys'), (0, 1, 'onesweep_pairs_default'),
                   (0, 1, 'bucket_pairs'), (0, 1, 'onesweep_pairs_wide'),
                   (0, 1, 'onesweep_pairs_default')]


NN = [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]
LR = NN + [[-2, 0, 0], [0, -3, 0], [0, 0, -3], [-3, 0, 0], [0, -9, 0], [0, 0, -9],
           [-4, 0, 0], [0, -27, 0], [0, 0, -27]]      # the project's 12-channel set (synthetic.LR_OFFSETS)


def _chan(offsets, adj_filter=1, have_bloom=0, skip_adj=1, nn=1):
    return 'chan %d %d %d %d %d ' % (adj_filter, have_bloom, skip_adj, nn, len(offsets)) + \
        ' '.join('%d %d %d' % tuple(o) for o in offsets)


def _chan_answers(plan, queries):
    out = []
    for a in plan(queries):
        v = [int(x) for x in a.split()]
        assert len(v) == 9 + v[8]
        out.append(dict(lr_mask=v[0], long_range=v[1], nn_ch=v[2:5], skip=v[5], nn3=v[6], nn_mix=v[7], loop=v[9:]))
    return out


def test_channels_nearest_neighbour_orders(plan):
    import itertools
    perms = list(itertools.permutations(range(3)))
    got = _chan_answers(plan, [_chan([NN[a] for a in p]) for p in perms])
    for p, g in zip(perms, got):
        # channel c carries axis p[c]: nn_ch[axis] is its position
        assert g == dict(lr_mask=0, long_range=0, nn_ch=[p.index(a) for a in range(3)], skip=1, nn3=1, nn_mix=0,
                         loop=[])


def test_channels_long_range_set(plan):
    with_bloom, without, nn_off, no_filter = _chan_answers(
        plan, [_chan(LR, have_bloom=1), _chan(LR), _chan(LR, have_bloom=1, nn=0), _chan(LR, adj_filter=0)])
    assert with_bloom == dict(lr_mask=0xFF8, long_range=1, nn_ch=[0, 1, 2], skip=1, nn3=0, nn_mix=1,
                              loop=list(range(3, 12)))
    # no Bloom filter: the long-range samples prove no adjacency, the markers stay
    assert (without['skip'], without['nn3'], without['nn_mix']) == (0, 0, 0)
    assert (nn_off['skip'], nn_off['nn3'], nn_off['nn_mix']) == (1, 0, 0)
    assert (no_filter['skip'], no_filter['nn3'], no_filter['nn_mix']) == (0, 0, 0)


def test_channels_missing_axis_and_repeats(plan):
    missing_lr, missing_3, repeat, positive, skip_off = _chan_answers(plan, [
        _chan([[-1, 0, 0], [0, -1, 0], [-2, 0, 0]], have_bloom=1),
        _chan([[-1, 0, 0], [0, -1, 0], [0, -1, 0]]),
        _chan(NN + [[0, -1, 0], [0, 0, -9]], have_bloom=1),
        _chan([[1, 0, 0], [0, -1, 0], [0, 0, -1]]),
        _chan(NN, skip_adj=0)])
    assert missing_lr == dict(lr_mask=4, long_range=1, nn_ch=[0, 1, -1], skip=0, nn3=0, nn_mix=0, loop=[2])
    assert missing_3 == dict(lr_mask=0, long_range=0, nn_ch=[0, 1, -1], skip=0, nn3=0, nn_mix=0, loop=[2])
    # a repeated nearest-neighbour offset: the first channel is the face channel, the repeat is looped
    assert repeat == dict(lr_mask=16, long_range=1, nn_ch=[0, 1, 2], skip=1, nn3=0, nn_mix=1, loop=[3, 4])
    assert positive['nn_ch'] == [-1, 1, 2] and positive['lr_mask'] == 0 and positive['nn3'] == 0
    assert (skip_off['skip'], skip_off['nn3']) == (0, 0)   # CTG_SKIP_ADJ=0


def _key_range(min_u, max_v, nb, ib):
    vmax = min(max_v, (1 << nb) - 1)
    kmax = (((vmax << nb) | vmax) << ib) | ((1 << ib) - 1)
    return min((min(min_u, vmax) << nb) << ib, kmax), kmax


def test_packed_key_range(plan):
    cases = [(0, 131071, 17, 23),          # min_u = 0
             (200000, 131071, 17, 23),     # min_u > max_v: clamped
             (70000, (1 << 17) - 1, 17, 23),   # max_v = 2^nb - 1
             (5, 1000, 10, 0),             # ib = 0
             (70000, 100000, 17, 23), (1, 1, 1, 1), (3, (1 << 20) - 1, 20, 23)]
    got = plan(['range %d %d %d %d' % c for c in cases])
    assert [tuple(map(int, g.split())) for g in got] == [_key_range(*c) for c in cases]
