"""The host layer's decisions (csrc/ctg_plan.h: call boxes, tile depths, the
batched-block plan, buffer sizes, channel classes, record-sort path, bucket
key range, bucket geometry of the two bucket sorts, ...) are pure functions; tools/plan_check.cpp
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


# ---------------------------------------------------------------------------
# the host decisions of the face-scan entry points.  The expected values are
# worked by hand or by the arithmetic restated here in Python, never printed
# from the code under test.
# ---------------------------------------------------------------------------
def _box(shape, begin=None, end=None, max_voxels=0):
    b, e = begin or (0, 0, 0), end or (0, 0, 0)
    return 'box %d %d %d %d %d %d %d %d %d %d %d %d' % (tuple(shape) + (int(begin is not None),) + tuple(b) +
                                                        (int(end is not None),) + tuple(e) + (max_voxels,))


def test_call_box(plan):
    cap = (1 << 32) - 1
    ok = [(_box((4, 5, 6)), (0, 0, 0, 4, 5, 6, 120)),
          (_box((4, 5, 6), begin=(1, 2, 3)), (1, 2, 3, 4, 5, 6, 3 * 3 * 3)),
          (_box((4, 5, 6), end=(2, 5, 1)), (0, 0, 0, 2, 5, 1, 10)),
          (_box((4, 5, 6), begin=(1, 2, 3), end=(1, 5, 6)), (1, 2, 3, 1, 5, 6, 0)),       # an empty box is a box
          (_box((0, 5, 6)), (0, 0, 0, 0, 5, 6, 0)),
          (_box((3, 5, 286331153), max_voxels=0), (0, 0, 0, 3, 5, 286331153, cap)),       # no cap
          (_box((3, 5, 286331152), max_voxels=cap), (0, 0, 0, 3, 5, 286331152, cap - 15))]
    for q, exp in ok:
        assert tuple(map(int, plan([q])[0].split())) == (0,) + exp, q
    outside = [_box((4, -5, 6)), _box((4, 5, 6), begin=(0, -1, 0)), _box((4, 5, 6), end=(4, 5, 7)),
               _box((4, 5, 6), begin=(3, 0, 0), end=(2, 5, 6)),
               _box((1 << 11, 1 << 11, 1 << 10), end=(1 << 11, 1 << 11, (1 << 10) + 1), max_voxels=cap)]
    assert [int(a.split()[0]) for a in plan(outside)] == [1] * len(outside)
    too_large = [_box((3, 5, 286331153), max_voxels=cap), _box((1 << 11, 1 << 11, 1 << 10), max_voxels=cap)]
    assert [int(a.split()[0]) for a in plan(too_large)] == [2, 2]


def test_vol_box(plan):
    """vol_box against numpy: the strides of a C-ordered array of the shape in
    elements, base the flat index of b, n = e - b; and through them every
    voxel of the box is the array element numpy's slice holds."""
    import numpy as np
    cases = [((3, 5, 7), (0, 0, 0), (3, 5, 7)),      # the whole array
             ((3, 5, 7), (1, 2, 3), (3, 4, 7)),      # off the origin on all three axes
             ((3, 5, 7), (2, 4, 6), (3, 5, 7)),      # one voxel, the last
             ((3, 5, 7), (1, 2, 3), (1, 4, 7)),      # empty
             ((3, 5, 7), (3, 5, 7), (3, 5, 7)),      # empty at the far corner
             ((5, 9, 13), (1, 2, 3), (4, 9, 12)),
             ((1, 1, 1), (0, 0, 0), (1, 1, 1))]
    got = plan(['volbox %d %d %d %d %d %d %d %d %d' % (s + b + e) for s, b, e in cases])
    for (shape, b, e), g in zip(cases, got):
        a = np.arange(shape[0] * shape[1] * shape[2], dtype=np.int64).reshape(shape)
        s_z, s_y, base, nz, ny, nx = map(int, g.split())
        assert (s_z, s_y, 1) == tuple(st // a.itemsize for st in a.strides), (shape, g)
        assert base == sum(x * st // a.itemsize for x, st in zip(b, a.strides)), (shape, b, g)   # b's flat index
        assert (nz, ny, nx) == tuple(hi - lo for lo, hi in zip(b, e)), (shape, b, e, g)
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
        assert np.array_equal(a.ravel()[base + z * s_z + y * s_y + x] if z.size else np.zeros((nz, ny, nx), np.int64),
                              a[b[0]:e[0], b[1]:e[1], b[2]:e[2]])


MAX_X = 1 << 30     # (the scan's own limit is the caller's: any value above the shapes used here)
UNIQUE_ROWS = 8


def _blk(shape, label_offset=0, data_offset=0, own=None, graph=None):
    own = own or ((0, 0, 0), shape)
    graph = graph or ((0, 0, 0), shape)
    return dict(shape=shape, label_offset=label_offset, data_offset=data_offset, own=own, graph=graph)


def _blocks_query(blocks, has_data=0, n_channels=0, labels_len=None, data_len=0, max_x=MAX_X, tile_z=0):
    if labels_len is None:
        labels_len = max(b['label_offset'] + b['shape'][0] * b['shape'][1] * b['shape'][2] for b in blocks)
    q = ['blocks %d %d %d %d %d %d %d %d %d' % (len(blocks), has_data, n_channels, labels_len, data_len, max_x,
                                                ROWS_WIDE, UNIQUE_ROWS, tile_z)]
    for b in blocks:
        q.append('%d %d' % (b['label_offset'], b['data_offset']))
        q += ['%d %d %d' % tuple(v) for v in (b['shape'], b['own'][0], b['own'][1], b['graph'][0], b['graph'][1])]
    return ' '.join(q)


def _ceil(a, b):
    return -(-a // b)


def _blocks_expected(blocks, tile_z=0):
    """The parent's inline arithmetic (ctg_rag_blocks), restated."""
    n = len(blocks)
    own, vox, zmax = 0, 0, 1
    for blk in blocks:
        o = 1
        for k in range(3):
            o *= max(0, blk['own'][1][k] - blk['own'][0][k])
        own += o
        vox += blk['shape'][0] * blk['shape'][1] * blk['shape'][2]
        zmax = max(zmax, blk['shape'][0])
    tz = tile_z if tile_z else min(zmax, 128)
    tag_bits = 0 if n - 1 <= 0 else max(1, (n - 1).bit_length())
    shift = 32 - tag_bits
    mask = (0xFFFFFFFF & ~((1 << shift) - 1)) if tag_bits else 0
    prefix, uprefix, tiles = [0], [0], []
    for blk in blocks:
        z, y, x = blk['shape']
        t = (_ceil(x, 64), _ceil(y, ROWS_WIDE), _ceil(z, tz))
        oe = [max(0, blk['own'][1][k] - blk['own'][0][k]) for k in range(3)]
        prefix.append(prefix[-1] + t[0] * t[1] * t[2])
        uprefix.append(uprefix[-1] + _ceil(oe[2], 64) * _ceil(oe[1], UNIQUE_ROWS) * _ceil(oe[0], 16))
        tiles += list(t)
    return [0, own, vox, tz, tag_bits, shift, mask] + prefix + uprefix + tiles


def test_block_plan_tables(plan):
    a = _blk((10, 40, 50), own=((1, 0, 0), (10, 40, 50)))
    b = _blk((11, 33, 70), label_offset=20000, own=((1, 1, 1), (11, 33, 70)), graph=((0, 0, 0), (11, 33, 70)))
    c = _blk((200, 65, 129), label_offset=45410)                       # shape[0] above 128: two tiles deep
    empty = _blk((4, 9, 9), label_offset=45410 + 200 * 65 * 129, own=((2, 3, 3), (2, 9, 9)))   # an empty owned box
    cases = [[a], [a, b], [a, b, c], [a, b, c, empty], [empty]]
    got = plan([_blocks_query(bl) for bl in cases])
    for bl, g in zip(cases, got):
        assert [int(v) for v in g.split()] == _blocks_expected(bl), bl
    # by hand: one block has no tag; 2 and 3 blocks take 1 and 2 tag bits
    one, two, three = ([int(v) for v in g.split()] for g in got[:3])
    assert one[1:7] == [9 * 40 * 50, 10 * 40 * 50, 10, 0, 32, 0]
    assert one[7:] == [0, 2,  0, 1 * 5 * 1,  1, 2, 1]     # 50 -> 1 x tile, 40 -> 2 y tiles of 32; own 9 x 40 x 50
    assert two[3:7] == [11, 1, 31, 0x80000000] and three[3:7] == [128, 2, 30, 0xC0000000]
    assert three[7:11] == [0, 2, 2 + 2 * 2 * 1, 6 + 3 * 3 * 2]         # 200 planes in tiles of 128: 2 deep
    four = [int(v) for v in got[3].split()]
    assert four[12 + 4] == four[12 + 3]                                # the empty owned box adds no node tile
    # CTG_TILE_Z
    g = plan([_blocks_query([a, b, c], tile_z=7)])[0]
    assert [int(v) for v in g.split()] == _blocks_expected([a, b, c], tile_z=7)
    assert int(g.split()[3]) == 7


def test_block_plan_errors(plan):
    ok = _blk((2, 4, 8))
    outside = [_blk((2, -4, 8)), _blk((2, 4, 8), own=((0, -1, 0), (2, 4, 8))), _blk((2, 4, 8), own=((0, 0, 0), (3, 4, 8))),
               _blk((2, 4, 8), graph=((-1, 0, 0), (2, 4, 8))), _blk((2, 4, 8), graph=((0, 0, 0), (2, 5, 8))),
               _blk((2, 4, MAX_X + 1), own=((0, 0, 0), (0, 0, 0)), graph=((0, 0, 0), (0, 0, 0)))]
    got = plan([_blocks_query([ok, ok, bad], labels_len=64) for bad in outside])
    assert got == ['1 2'] * len(outside)
    arena = [dict(blocks=[ok, _blk((2, 4, 8), label_offset=-1)], labels_len=64),
             dict(blocks=[ok, _blk((2, 4, 8), label_offset=1)], labels_len=64),
             dict(blocks=[ok, _blk((2, 4, 8), data_offset=-1)], labels_len=64, has_data=1, data_len=64),
             dict(blocks=[ok, ok], labels_len=64, has_data=1, data_len=63),
             dict(blocks=[ok, ok], labels_len=64, has_data=1, n_channels=3, data_len=191)]
    got = plan([_blocks_query(**kw) for kw in arena])
    assert got == ['2 1', '2 1', '2 1', '2 0', '2 0']
    # without a data arena the data offsets are not looked at; the box before the arena; blocks in order
    fine = plan([_blocks_query([_blk((2, 4, 8), data_offset=-5)], labels_len=64)])[0]
    assert fine.split()[0] == '0'
    both = _blk((2, 4, 8), label_offset=-1, own=((0, 0, 0), (3, 4, 8)))
    assert plan([_blocks_query([both], labels_len=64),
                 _blocks_query([_blk((2, 4, 8), label_offset=1), both], labels_len=64)]) == ['1 0', '2 0']
    # 2^31 - 1 tiles fit one launch, one more does not (x tiles of 64: 2^24 - 1 wide tiles a row)
    wide = _blk((128, 32, 64 * ((1 << 24) - 1)), own=((0, 0, 0), (0, 0, 0)))
    many = [wide] * 128                                                  # 2^31 - 128 tiles
    row = _blk((127, 32, 64), own=((0, 0, 0), (0, 0, 0)))               # one tile each
    lens = dict(labels_len=1 << 62, max_x=1 << 40)
    got = plan([_blocks_query(many + [row] * 127, **lens), _blocks_query(many + [row] * 128, **lens)])
    assert got[0].split()[0] == '0' and got[1].split()[0] == '3'


def test_record_and_candidate_sizes(plan):
    V0 = 24 << 16                                                        # V / 24 = 2^16: the floor
    q = ['recfirst 0 0', 'recfirst 0 %d' % (V0 - 24), 'recfirst 0 %d' % V0, 'recfirst 0 %d' % (V0 + 24),
         'recfirst 0 %d' % (V0 + 24 * 64), 'recfirst 100000 %d' % V0, 'recfirst 0 %d' % (512 ** 3),
         'recgrow 0', 'recgrow 1000', 'recgrow 1001', 'recgrow 4000000',
         'cand 0', 'cand 1', 'cand 65535', 'cand 65536', 'cand 524288', 'cand 524296', 'cand 8000000',
         'candgrow 70000 9223372036854775807', 'candgrow 70000 70500', 'candgrow 70000 80000']
    exp = [65536, 65536, 65536, 65600, 65600, 100032, 5592448,           # rounded up to a multiple of 64
           1024 * 64, (1250 + 1024) * 64, (1251 + 1024) * 64, (5000000 + 1024) * 64,
           1, 1, 65535, 65536, 65536, 65537, 1000000,
           71024, 70500, 71024]
    assert [int(v) for v in plan(q)] == exp
    assert 5592448 == _ceil(512 ** 3 // 24, 64) * 64 and 100032 == _ceil(100000, 64) * 64


def test_bloom_blocks(plan):
    """48 bits an edge in 512-bit blocks, a power of two, 128 blocks at least:
    128 * 512 / 48 = 1365.33 edges fill the floor."""
    ns = [0, 1, 1365, 1366, 2730, 2731, 1000000]
    exp = []
    for n in ns:
        blocks = 128
        while blocks * 512 < n * 48:
            blocks *= 2
        exp.append(blocks)
    assert exp[:6] == [128, 128, 128, 256, 256, 512] and exp[6] == 131072
    assert [int(v) for v in plan(['bloom %d' % n for n in ns])] == exp


def test_narrow_rows_and_need_adj(plan):
    big = 1 << 28
    q = ['narrow 1 %d -1' % (big - 1), 'narrow 1 %d -1' % big, 'narrow 0 %d -1' % big, 'narrow 0 %d 1' % big,
         'narrow 1 1000 0', 'narrow 1 1000 1', 'narrow 1 %d 0' % big, 'narrow 1 %d 1' % big, 'narrow 1 1000 5']
    assert [int(v) for v in plan(q)] == [0, 2, 0, 0, 0, 1, 0, 1, 1]
    # need_adj of a whole array: n_channels, skip_adj_marks, adj_filter, have_bloom
    q = ['adj 0 0 1 0', 'adj 3 1 1 0', 'adj 3 0 1 0', 'adj 3 0 0 0', 'adj 12 1 1 1', 'adj 12 0 1 1', 'adj 0 0 0 0',
         'adjblocks 0', 'adjblocks 3']
    assert [int(v) for v in plan(q)] == [0, 0, 1, 2, 1, 1, 0, 0, 1]


def test_fold_regions(plan):
    rc = [(7 * r * r + 3) % 1000 for r in range(64)]
    rc[5] = 0
    rc[40] = 123456
    big = [1 << 26] * 64                                                 # total 2^32: the prefix wraps, the total does not
    got = plan(['fold ' + ' '.join(map(str, c)) for c in (rc, [0] * 64, big)])
    for c, g in zip((rc, [0] * 64, big), got):
        v = [int(x) for x in g.split()]
        off = [sum(c[:r]) & 0xFFFFFFFF for r in range(65)]
        assert v == [sum(c), max(c)] + off
    assert int(got[2].split()[0]) == 1 << 32 and int(got[2].split()[-1]) == 0


def test_exchange_counts(plan):
    world, row_words = 3, 28
    counts = [[(10 * s + d + 1, 100 * s + 7 * d) for d in range(world)] for s in range(world)]    # [src][dst]: rows, nodes
    flat = ' '.join('%d %d' % counts[s][d] for s in range(world) for d in range(world))
    q, exp = [], []
    for rank in range(world):
        rows = sum(counts[rank][d][0] for d in range(world))
        nodes = sum(counts[rank][d][1] for d in range(world))
        send = sum(counts[rank][d][0] * row_words + counts[rank][d][1] for d in range(world) if d != rank)
        recv = sum(counts[s][rank][0] * row_words + counts[s][rank][1] for s in range(world) if s != rank)
        q += ['xchg %d %d %d 0 %s' % (world, rank, row_words, flat), 'xchg %d %d %d 1 %s' % (world, rank, row_words, flat)]
        exp += [(rows, nodes, send), (rows, nodes, recv)]
    assert [tuple(map(int, g.split())) for g in plan(q)] == exp
    assert exp[0] == (1 + 2 + 3, 0 + 7 + 14, (2 + 3) * 28 + 7 + 14)      # rank 0 by hand
    assert plan(['xchg 1 0 28 0 5 9', 'xchg 1 0 28 1 5 9']) == ['5 9 0', '5 9 0']     # one rank: nothing moves


import exchange_plans as XP  # noqa: E402


def _xplan(plan, name, ranks=None):
    world, counts = XP.MATRICES[name]
    ranks = range(world) if ranks is None else ranks
    got = plan(['xplan %d %d %s' % (world, r, XP.flat(counts)) for r in ranks])
    return [[int(x) for x in g.split()] for g in got], got


def test_exchange_plan_matches_restatement(plan):
    """exchange_plan of every rank of every matrix of tests/exchange_plans.py,
    field by field against the restatement in Python integers."""
    for name, (world, counts) in XP.MATRICES.items():
        got, _ = _xplan(plan, name)
        for r in range(world):
            assert got[r] == XP.restate(counts, world, r)[0], (name, r)


def test_exchange_plan_by_hand(plan):
    (w1,), _ = _xplan(plan, 'world1')
    assert w1 == [0, 5, 0, 9, 5, 9, 0, 0] + [0, 0, 0, 0] * 2            # one rank: own range only, no segment
    # world 3, counts[s][d] = (10s + d + 1, 100s + 7d), rank 0: keeps (1, 0); sends (2, 7) to 1 and (3, 14) to 2,
    # which start at row 1 / node 0 and row 3 / node 7 of its table; receives (11, 100) from 1 and (21, 200) from 2
    (r0,), _ = _xplan(plan, 'world3', [0])
    assert r0 == [0, 1, 0, 0, 6, 21, 1, 0,
                  2, 0, 0, 0, 2, 7, 63, 5, 21, 161, 1, 0, 3, 7,
                  2, 0, 0, 0, 11, 100, 408, 32, 300, 1196, 0, 0, 0, 0]
    for name in ('diagonal',):                                           # nothing to exchange, on every rank
        got, _ = _xplan(plan, name)
        assert all(g[6] == 0 and g[8:] == [0, 0, 0, 0] * 2 for g in got)
    got, _ = _xplan(plan, 'only_to_last')
    assert [g[6] for g in got] == [1] * 5                                # the same answer on every rank
    assert got[1][8:13] == [1, 0, 0, 0, 7] and got[4][-9:] == [1, 0, 0, 0, 7, 1, 7 * 28 + 1, 0, 0]
    assert all(g[8] == 0 for i, g in enumerate(got) if i != 1)           # nobody else sends
    # a destination with nodes and no rows keeps its segment; one with neither has none
    assert _xplan(plan, 'nodes_only_between', [0])[0][0][8:20] == [3, 0, 0, 0, 3, 2, 86, 3, 6, 90, 8, 7]
    assert _xplan(plan, 'empty_between', [0])[0][0][8:17] == [2, 0, 0, 0, 3, 2, 86, 8, 3]
    assert _xplan(plan, 'empty_own', [1])[0][0][:4] == [2, 0, 2, 0]
    got, _ = _xplan(plan, 'world32_full', [0, 31])
    assert got[0][8] == 31 and got[1][8] == 31                           # 31 segments each way


def test_exchange_plan_thresholds(plan):
    """M, e_cnt + M and NM against 2^32, at the bound and one below."""
    for what in ('rows', 'slots', 'nodes'):
        assert _xplan(plan, what + '_at_bound', [0])[0][0][7] == 1
        assert _xplan(plan, what + '_below_bound', [0])[0][0][7] == 0
    assert _xplan(plan, 'slots_at_bound', [1])[0][0][7] == 0             # the other rank receives nothing


def _segof(prefix, i):
    return 'segof %d %d %s' % (i, len(prefix) - 1, ' '.join(map(str, prefix)))


def test_seg_of(plan):
    """seg_of at the first and last element of every non-empty segment of
    every prefix table of the matrices, and on tables made by hand: one
    segment, 32 segments, and equal consecutive prefixes (empty segments)."""
    tables = [[0, 5], [0, 1], list(range(33)), [3 * i * i for i in range(33)],
              [0, 3, 3, 3, 7], [0, 0, 4], [0, 4, 4], [0, 0, 0, 1], [0, 2, 2, 5, 5, 5, 6, 6]]
    for name, (world, counts) in XP.MATRICES.items():
        if name.endswith('bound'):
            continue
        for line in _xplan(plan, name)[1]:
            tables += [p for n, p in XP.prefixes(line) if n and p[-1]]
    q, exp = [], []
    for p in tables:
        n = len(p) - 1
        for s in range(n):
            if p[s] < p[s + 1]:
                q += [_segof(p, p[s]), _segof(p, p[s + 1] - 1)]
                exp += [s, s]
        q += [_segof(p, 0), _segof(p, p[-1] - 1)]
        exp += [min(s for s in range(n) if p[s + 1] > 0), max(s for s in range(n) if p[s] < p[-1])]
    assert any(len(p) == 2 for p in tables) and any(len(p) == 33 for p in tables)
    assert len(q) > 1000
    assert [int(g) for g in plan(q)] == exp


def test_slab_range(plan):
    """slab_range on the cases of test_dist_cpu.py::test_mgpu_slab_plan_c_abi:
    owned ranges tile [0, Z) in rank order, the halo below reaches as far as
    the faces / offsets (clipped at plane 0), and the reach above is reported."""
    nn = [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]
    lr = nn + [[-2, 0, 0], [0, -3, 0], [0, 0, -3], [-3, 0, 0], [0, -9, 0], [0, 0, -9], [-4, 0, 0], [0, -27, 0], [0, 0, -27]]
    for Z, world in [(1024, 1), (2048, 8), (101, 4), (7, 7)]:
        for offs, down in [([], 1), (nn, 1), (lr, 4)]:
            tail = '%d %s' % (len(offs), ' '.join(str(v) for o in offs for v in o))
            got = [[int(x) for x in g.split()] for g in plan(['slab %d %d %d %s' % (Z, world, r, tail) for r in range(world)])]
            assert got[0][2:4] == [0, 0] and got[-1][4] == Z
            for r, (dn, up, rd, own, end) in enumerate(got):
                assert (dn, up) == (down, 0)
                assert own == Z * r // world and end == Z * (r + 1) // world and end > own
                assert own - rd == (min(down, own) if r else 0)
    assert plan(['slab 64 2 0 1 1 0 0', 'slab 64 1 0 2 5 0 0 -2 0 0']) == ['1 1 0 0 32', '2 5 0 0 64']


# ---------------------------------------------------------------------------
# bucket geometry of the group sort and of the packed-key bucket sort
# (plan_group_sort, plan_bucket_keys, gs_bucket_of, gs_bucket_key) against
# tests/sort_plan.py, the rules restated in Python integers
# ---------------------------------------------------------------------------
import sort_plan as SP  # noqa: E402

WHY = {name: i for i, name in enumerate(SP.DECLINES)}


def _label_ranges(nb):
    """[lo, hi] label ranges of 2, 16, 1000 labels and the full range, at the
    bottom, at the top and across the middle of [0, 2^nb)."""
    size = 1 << nb
    out = set()
    for width in (2, 16, 1000, size):
        w = min(width, size)
        for lo in (0, size - w, max(0, min(size - w, size // 2 - w // 2))):
            out.add((lo, lo + w - 1))
    return sorted(out)


def _gs_n_values(nb, ub, lo, hi):
    """1 .. 2^32 - 1, and for every shift the record counts that put the
    average bucket at GS_TARGET exactly and one record above it."""
    ns = {1, 2, SP.GS_TARGET, SP.GS_TARGET + 1, 100000, 1 << 20, 1 << 31, (1 << 32) - 1}
    kmin, kmax = SP.key_range(nb, ub, lo, hi)
    for s in range(ub + nb, -1, -1):
        c = (kmax >> s) - (kmin >> s) + 1
        if c > SP.GS_M:
            break
        ns.update(n for n in (SP.GS_TARGET * c - 1, SP.GS_TARGET * c, SP.GS_TARGET * c + 1) if 0 < n < (1 << 32))
    return sorted(ns)


@pytest.fixture(scope='module')
def gs_sweep(plan):
    """(inputs, the plan's answer) for the whole sweep: nb 1 .. 32 (ub = nb, as
    whole arrays sort; kb = 64 at nb = 32), every label range, two slot widths."""
    cases = []
    for nb in range(1, 33):
        for lo, hi in _label_ranges(nb):
            for n in _gs_n_values(nb, nb, lo, hi):
                for ib in (16, 28):
                    cases.append((n, nb, nb, ib, lo, hi))
    # block-tagged geometry for completeness: u has 32 bits whatever the labels
    cases += [(n, nb, 32, 20, lo, hi) for nb in (9, 20, 31) for lo, hi in _label_ranges(nb) for n in (5, 1 << 22)]
    got = plan(['gsort %d %d %d %d %d %d' % c for c in cases])
    return cases, [[int(v) for v in g.split()] for g in got]


def test_group_sort_plan_matches_rule(gs_sweep):
    cases, got = gs_sweep
    seen = set()
    for c, g in zip(cases, got):
        exp = SP.plan_group_sort(*c)
        seen.add(exp['why'])
        assert g[0] == WHY[exp['why']], (c, g, exp)
        if 'shift' in exp:
            assert g[1:] == [exp['shift'], exp['nbk'], exp['bk0'], exp['min_pk'], exp['max_pk']], (c, g, exp)
        else:
            assert g[1] == -1, (c, g)
    assert seen == {'none', 'key_bits', 'item_bits', 'low_bits'}
    assert len(cases) > 10000


def test_group_sort_plan_declines(plan):
    """The reasons in their order: the record count first, then the key bits,
    then the item and the low key bits."""
    q = ['gsort 0 20 20 16 0 1000', 'gsort -1 20 20 16 0 1000', 'gsort 4294967296 20 20 16 0 1000',
         'gsort 0 32 32 16 0 4294967295',           # n before kb
         'gsort 5 32 32 16 0 4294967295', 'gsort 5 33 31 16 0 4294967295', 'gsort 5 31 33 16 0 2147483647',
         'gsort 5 32 31 16 0 4294967295',           # 63 key bits pass; one bucket of 2^63 keys + 16 slot bits
         'gsort 5 31 31 2 0 2147483647',            # 62 key bits, 5 records: one bucket of 2^62 keys (fits with 2 slot bits)
         'gsort 5 20 20 40 0 1000000',              # shift 40 + 40 slot bits
         'gsort 4294967295 31 31 16 2147483000 2147483647']
    got = [[int(v) for v in g.split()] for g in plan(q)]
    assert [g[0] for g in got] == [1, 1, 1, 1, 2, 2, 2, 3, 4, 3, 0]
    assert all(g[1] == -1 and g[2:] == [0, 0, 0, 0] for g in got[:7])
    assert got[7][1:3] == [63, 1] and got[8][1:3] == [62, 1]


def _sample_keys(kmin, kmax, shift, bk0, nbk):
    ks = {kmin, kmax}
    ks.update(kmin + (kmax - kmin) * k // 7 for k in range(1, 7))
    for j in (1, nbk // 2, nbk - 1):     # both sides of a bucket boundary
        edge = (bk0 + j) << shift
        ks.update(k for k in (edge - 1, edge) if kmin <= k <= kmax)
    return sorted(ks)


def _check_bucket_keys(plan, plans, max_buckets):
    """For every (kmin, kmax, shift, bk0, nbk): the smallest key in bucket 0,
    the largest in the last one, and every sampled key's bucket bits rebuilt
    from its bucket.  Returns the largest (kmax >> shift) met."""
    queries, expect = [], []
    top = 0
    for kmin, kmax, shift, bk0, nbk in sorted(plans):
        assert 1 <= nbk <= max_buckets and bk0 == kmin >> shift and nbk == (kmax >> shift) - bk0 + 1
        top = max(top, kmax >> shift)
        for k in _sample_keys(kmin, kmax, shift, bk0, nbk):
            queries.append('gskey %d %d %d' % (k, shift, bk0))
            expect.append(((k >> shift) - bk0, (k >> shift) << shift, k == kmin, k == kmax, nbk))
    got = plan(queries)
    for q, g, (b, key, first, last, nbk) in zip(queries, got, expect):
        gb, gkey = (int(v) for v in g.split())
        assert gb == b and 0 <= gb < nbk, (q, g, b)
        assert not first or gb == 0, (q, g)
        assert not last or gb == nbk - 1, (q, g)
        assert gkey == key, 'bucket bits rebuilt wrong: %s -> %s, expected %d' % (q, g, key)
    return top


def test_group_sort_bucket_key_rebuild(plan, gs_sweep):
    """Every accepted plan of the sweep: at most GS_M buckets, min_pk in bucket
    0, max_pk in bucket nbk - 1, and gs_bucket_key(gs_bucket_of(pk)) == (pk >>
    shift) << shift at both ends, between them and on both sides of bucket
    boundaries -- also where pk >> shift needs more than 32 bits (labels near
    2^30 and above with many records a label), which the sweep must contain."""
    cases, got = gs_sweep
    plans = {(g[4], g[5], g[1], g[3], g[2]) for g in got if g[0] == 0}
    assert len(plans) > 1000
    top = _check_bucket_keys(plan, plans, SP.GS_M)
    assert top >= 1 << 32
    # bk0 below 2^32 and b + bk0 above it; and bk0 itself above 2^32
    assert any(bk0 < (1 << 32) <= bk0 + nbk - 1 for _, _, _, bk0, nbk in plans)
    assert any(bk0 >= (1 << 32) for _, _, _, bk0, _ in plans)


def test_group_sort_record_heavy_labels_near_2_30(plan):
    """The volumes of tests/test_gpu_label_widths.py, by the plan alone: 16
    (5) labels from 2^30 with 7168 (8192) records a face reach shift 29, where
    the bucket index passes 2^32; 16 labels from 2^29 stay below it."""
    q = ['gsort %d 31 31 16 %d %d' % (15 * 7168, 1 << 30, (1 << 30) + 15),
         'gsort %d 31 31 16 %d %d' % (4 * 8192, 1 << 30, (1 << 30) + 4),
         'gsort %d 31 31 16 %d %d' % (15 * 7168, (1 << 30) - 8, (1 << 30) + 7),
         'gsort %d 30 30 16 %d %d' % (15 * 7168, 1 << 29, (1 << 29) + 15)]
    got = [[int(v) for v in g.split()] for g in plan(q)]
    assert [g[:2] for g in got] == [[0, 29], [0, 29], [0, 29], [0, 28]]
    assert [(g[5] >> g[1]) >= (1 << 32) for g in got] == [True, True, True, False]
    assert got[2][3] < (1 << 32) <= got[2][3] + got[2][2] - 1      # bk0 fits 32 bits, bk0 + b does not
    _check_bucket_keys(plan, {(g[4], g[5], g[1], g[3], g[2]) for g in got}, SP.GS_M)


def test_bucket_keys_plan(plan):
    """plan_bucket_keys over packed-key ranges (packed_key_range of label
    ranges, slot bits 0 / 16 / 23) and record counts around every bucket-bit
    step: the rule's shift, at most 2^BK_MAX_BITS buckets, kmin in bucket 0,
    kmax in the last, bucket bits rebuilt."""
    ns = sorted({1, 1023, (1 << 32) - 1} | {(1 << b) + d for b in range(10, 23) for d in (-1, 0)})
    cases = []
    for ib in (0, 16, 23):
        for nb in range(1, (63 - ib) // 2 + 1):
            for lo, hi in _label_ranges(nb):
                kmin, kmax = _key_range(lo, hi, nb, ib)
                cases += [(n, ib, ib + 2 * nb, kmin, kmax) for n in ns]
    got = [[int(v) for v in g.split()] for g in plan(['bkeys %d %d %d %d %d' % c for c in cases])]
    plans = set()
    for c, g in zip(cases, got):
        exp = SP.plan_bucket_keys(*c)
        assert g == [1, exp['bb'], exp['shift'], exp['nbk'], exp['bk0']], (c, g, exp)
        assert g[3] <= 1 << g[1] <= 1 << SP.BK_MAX_BITS and c[1] <= g[2] <= c[2] - g[1]
        plans.add((c[3], c[4], g[2], g[4], g[3]))
    assert len(cases) > 10000 and {g[1] for g in got} == set(range(1, SP.BK_MAX_BITS + 1))
    assert _check_bucket_keys(plan, plans, 1 << SP.BK_MAX_BITS) >= 1 << 32
    bad = ['bkeys 0 0 20 0 5', 'bkeys 4294967296 0 20 0 5', 'bkeys 5 0 65 0 5', 'bkeys 5 -1 20 0 5', 'bkeys 5 20 20 0 5',
           'bkeys 5 0 20 6 5', 'bkeys 5000000 0 20 0 %d' % (1 << 40)]      # (the last: kmax past 2^hi_bit)
    assert [g.split()[0] for g in plan(bad)] == ['0'] * len(bad)
