"""The face scan's interior predicate (csrc/ctg_plan.h: scan_wave_interior) on
the CPU.  tools/scan_interior_check.cpp -- built with the host compiler and
-fsanitize=address,undefined -- sweeps it against the plane loop's masks and
clamps, evaluated per lane, row and plane as k_face_scan defines them: a wave
is interior iff every mask is full and every clamp is the identity.  Shapes
around the tile edges (X in 63, 64, 65, 128, 129; Y in 31, 32, 33, 36, 37; Z in
1 .. 5 with tiles 1, 2 and 4 planes deep), owned boxes that start and end on
and off the array's edges and the tile edges, 4 and 1 rows a wave.  The
closed-form count of a launch's interior waves (scan_interior_waves, what
ctg_last_scan reports) is compared with the count over the waves, without and
with tail tiles."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def check(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('interior') / 'scan_interior_check')
    subprocess.run([cxx, '-std=c++17', '-O2', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    os.path.join(ROOT, 'tools', 'scan_interior_check.cpp'), '-o', exe],
                   check=True, capture_output=True, timeout=300)

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        return r.stdout.split()
    return run


def test_sweep_matches_the_masks(check):
    out = check()
    got = dict(zip(out[0::2], map(int, out[1::2])))
    assert got['mismatches'] == 0
    assert got['waves'] > 10 ** 7 and got['launches'] > 10 ** 5
    assert 0 < got['interior'] < got['waves'] // 10   # both answers occur


def _wave(check, shape, x0, yw, rows, z0, z1, own_begin=(0, 0, 0), own_end=None):
    pred, masks = map(int, check(*shape, *own_begin, *(own_end or shape), x0, yw, rows, z0, z1))
    assert pred == masks
    return bool(pred)


def test_full_tiles_at_the_array_edge_are_not_interior(check):
    """4 x 64 x 128 with two-plane tiles: exact multiples of the 64 x 32 x 2
    tile.  Every tile is full; only those with a neighbour above on every axis
    are interior."""
    shape = (4, 64, 128)
    assert _wave(check, shape, 0, 0, 4, 0, 2)
    assert _wave(check, shape, 0, 28, 4, 0, 2)        # last wave of y tile 0: its halo row is y tile 1's
    assert not _wave(check, shape, 64, 0, 4, 0, 2)    # last x tile: no column 128
    assert not _wave(check, shape, 0, 60, 4, 0, 2)    # last wave of the last y tile: no row 64
    assert _wave(check, shape, 0, 56, 4, 0, 2)        # ... the wave before it has one
    assert not _wave(check, shape, 0, 0, 4, 2, 4)     # last z layer: no plane 4


def test_one_past_the_tile(check):
    """5 x 33 x 65: one voxel, one row and one plane beyond the first tile --
    exactly what its last lane, last wave and last plane need above them."""
    shape = (5, 33, 65)
    assert _wave(check, shape, 0, 28, 4, 0, 2) and _wave(check, shape, 0, 0, 4, 2, 4)
    assert not _wave(check, shape, 64, 0, 4, 0, 2)
    assert not _wave(check, shape, 0, 32, 4, 0, 2)
    assert not _wave(check, shape, 0, 0, 4, 4, 5)
    assert not _wave(check, (5, 32, 65), 0, 28, 4, 0, 2)
    assert not _wave(check, (5, 33, 64), 0, 0, 4, 0, 2)
    assert not _wave(check, (4, 33, 65), 0, 0, 4, 2, 4)


def test_owned_box_inside_the_array(check):
    """A slab with a halo plane: the layer that holds plane 0 is not interior.
    An owned box that ends before the array does cuts the same way."""
    shape = (5, 37, 131)
    assert not _wave(check, shape, 0, 0, 4, 0, 2, own_begin=(1, 0, 0))
    assert _wave(check, shape, 0, 0, 4, 2, 4, own_begin=(1, 0, 0))
    assert _wave(check, shape, 64, 0, 4, 0, 2)                                # column 128 exists
    assert not _wave(check, shape, 64, 0, 4, 0, 2, own_end=(5, 37, 128))      # ... but is not owned
    assert not _wave(check, shape, 0, 0, 4, 0, 2, own_begin=(0, 1, 0))
    assert not _wave(check, shape, 0, 0, 1, 0, 2, own_begin=(0, 1, 0))        # narrow: one row a wave
    assert _wave(check, shape, 0, 1, 1, 0, 2, own_begin=(0, 1, 0))
