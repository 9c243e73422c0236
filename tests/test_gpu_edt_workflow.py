"""The two job bodies that sit on the morphology table, through the harness:
morphology_workflow -> region_centers_workflow and morphology_workflow ->
object_distances_workflow on a synthetic label volume, against a numpy and
scipy restatement of the two reference bodies (morphology/region_centers.py:
106-133, distances/object_distances.py:109-180) written here; and apply_dt of
the watershed on the same volume's boundary map."""
import pickle

import numpy as np
import pytest
from numpy.testing import assert_array_equal
from scipy import ndimage as ndi

from cluster_tools_amd import distance, n5, rag
from harness import workflow

pytestmark = pytest.mark.gpu

SHAPE, BLOCK = (24, 48, 48), (16, 32, 32)


@pytest.fixture(scope='module')
def volume(gpu):
    """(labels, boundary): consecutive labels 1 .. n of a cell-10 synthetic
    volume, plus one box-shaped object that fills its bounding box."""
    lab, bnd = rag.synth_volume(SHAPE, cell=10, seed=11)
    _, seg = np.unique(lab.cpu().numpy(), return_inverse=True)
    seg = (seg.reshape(SHAPE) + 1).astype(np.uint64)
    seg[3:8, 5:12, 30:37] = seg.max() + 1
    assert 40 < seg.max() < 400
    return seg, bnd.cpu().numpy()


@pytest.fixture(scope='module')
def files(volume, tmp_path_factory):
    """The label volume and its morphology table on disk, computed once."""
    seg = volume[0]
    d = tmp_path_factory.mktemp('edt_wf')
    path, out = str(d / 'in.n5'), str(d / 'out.n5')
    with n5.File(path) as f:
        f.create_dataset('seg', shape=SHAPE, chunks=BLOCK, dtype='uint64', compression='gzip')[:] = seg
    workflow.morphology_workflow(path, 'seg', out, 'morphology', BLOCK, int(seg.max()), max_jobs=2)
    with n5.File(out, 'r') as f:
        morphology = f['morphology'][:]
    return path, out, morphology, str(d)


def boxes(seg):
    """Inclusive bounding boxes per label from numpy: (n_labels, 3) min and max."""
    n = int(seg.max()) + 1
    lo, hi = np.zeros((n, 3), dtype=np.uint64), np.zeros((n, 3), dtype=np.uint64)
    for l, sl in enumerate(ndi.find_objects(seg.astype(np.int64)), start=1):
        if sl is not None:
            lo[l] = [s.start for s in sl]
            hi[l] = [s.stop - 1 for s in sl]
    return lo, hi


@pytest.mark.parametrize('resolution', [(1, 1, 1), (4, 1, 1)], ids=['iso', 'aniso'])
def test_region_centers_workflow(volume, files, resolution):
    seg = volume[0]
    path, out, morphology, _ = files
    lo, hi = boxes(seg)
    assert_array_equal(morphology[:, 5:8].astype(np.uint64), lo)
    assert_array_equal(morphology[:, 8:11].astype(np.uint64), hi)
    n_labels, ignore = int(seg.max()) + 1, 7
    key = 'centers_%d' % resolution[0]
    workflow.region_centers_workflow(path, 'seg', out, 'morphology', out, key, n_labels - 1, ignore_label=ignore,
                                     resolution=resolution, id_chunks=30, max_jobs=2)
    with n5.File(out, 'r') as f:
        assert f[key].shape == (n_labels, 3) and tuple(f[key].chunks) == (30, 3) and f[key].dtype == np.float32
        got = f[key][:]
    # the reference body, restated: the stop is the inclusive maximum, as upstream slices it
    want = np.zeros((n_labels, 3), dtype=np.float32)
    filled = 0
    for label_id in range(n_labels):
        if label_id == ignore:
            continue
        bb = tuple(slice(int(a), int(b)) for a, b in zip(lo[label_id], hi[label_id]))
        obj = seg[bb] == label_id
        if obj.sum() == 0:
            continue
        filled += bool(obj.all())
        center = np.unravel_index(np.argmax(ndi.distance_transform_edt(obj, sampling=resolution)), obj.shape)
        want[label_id] = [c + b.start for c, b in zip(center, bb)]
    assert filled >= 1                                            # the box-shaped object: scipy's last-voxel accident
    assert not want[ignore].any() and not want[0].any() and np.count_nonzero(want.any(axis=1)) > 30
    assert_array_equal(got, want)


def reference_object_distances(seg, lo, hi, label_id, max_distance, resolution):
    """distances/object_distances.py:109-180 with scipy's transform for vigra's."""
    def labels_and_distances(bb):
        labels = seg[bb]
        return labels, ndi.distance_transform_edt(labels != label_id, sampling=resolution).astype(np.float32)

    def face_minima(d):
        return [d[0].min(), d[-1].min(), d[:, 0].min(), d[:, -1].min(), d[:, :, 0].min(), d[:, :, -1].min()]

    bb = tuple(slice(int(a), int(b) + 1) for a, b in zip(lo[label_id], hi[label_id]))
    labels, dist = labels_and_distances(bb)
    faces = face_minima(dist)
    enlarged = False
    if min(faces) < max_distance:
        new = []
        for dim, b in enumerate(bb):
            start, stop = b.start, b.stop
            if faces[2 * dim] < max_distance:
                start = max(start - (max_distance - faces[2 * dim]) / resolution[dim], 0)
            if faces[2 * dim + 1] < max_distance:
                stop = min(stop + (max_distance - faces[2 * dim + 1]) / resolution[dim], seg.shape[dim])
            new.append(slice(int(start), int(stop)))
        enlarged = tuple(new) != bb
        labels, dist = labels_and_distances(tuple(new))
    out = {}
    for obj in np.unique(labels):
        if obj != 0 and label_id < obj:
            v = dist[labels == obj].min()
            if v < max_distance:
                out[(label_id, int(obj))] = v
    return out, enlarged


@pytest.mark.parametrize('resolution', [(1, 1, 1), (4, 1, 1)], ids=['iso', 'aniso'])
def test_object_distances_workflow(volume, files, resolution):
    seg = volume[0]
    path, out, _, tmp = files
    lo, hi = boxes(seg)
    n_labels, max_distance = int(seg.max()) + 1, 3.5
    pkl = '%s/distances_%d.pkl' % (tmp, resolution[0])
    workflow.object_distances_workflow(path, 'seg', out, 'morphology', pkl, n_labels - 1, max_distance,
                                       resolution=resolution, id_chunks=30, max_jobs=2)
    with open(pkl, 'rb') as f:
        got = pickle.load(f)
    want, grown = {}, []
    for label_id in range(1, n_labels):
        d, enlarged = reference_object_distances(seg, lo, hi, label_id, max_distance, resolution)
        want.update(d)
        grown.append(enlarged)
    # a tight box has the object on every face: it grows wherever the volume leaves room
    assert any(grown) and len(want) > 50
    assert set(got) == set(want)
    for k, v in want.items():
        assert type(got[k]) is np.float32 and got[k] == v, k


def test_apply_dt_on_the_boundary_map(volume):
    bnd = volume[1]
    above = bnd > np.float32(0.5)
    assert above.any(axis=(1, 2)).all() and not above.all()
    got = distance.apply_dt(bnd, threshold=.5)
    for z in range(SHAPE[0]):
        assert_array_equal(got[z], ndi.distance_transform_edt(~above[z]).astype(np.float32))
    for pitch in (None, (4, 1, 1)):
        got = distance.apply_dt(bnd, threshold=.5, pixel_pitch=pitch, apply_dt_2d=False)
        assert_array_equal(got, ndi.distance_transform_edt(~above, sampling=pitch).astype(np.float32))
    assert distance.apply_dt(bnd, threshold=float(bnd.max())) is None
    assert distance.apply_dt(bnd, threshold=float(bnd.max()), apply_dt_2d=False) is None
