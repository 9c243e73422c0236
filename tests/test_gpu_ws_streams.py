"""ctg_seeded_watershed held to its stream, off the null stream: Protocol A of
tests/test_gpu_streams.py (a decoy warm-up, the null stream held busy, the true
input staged on the side stream behind a delay) for the plain flood, the size
filter with its nested morphology scan and second flood, the 2-D mode, and one
host-memory case with an explicit ``stream=``."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from cluster_tools_amd import rag                      # noqa: E402
from tests import ws_cases as W                        # noqa: E402

import stream_cases as SC                              # noqa: E402
from test_gpu_streams import Case, protocol_a         # noqa: E402

SHAPE = (9, 37, 70)        # off the grid on every axis, two workgroups and more


@pytest.fixture(scope='module')
def side(gpu):
    return SC.side_stream()


class Watershed(Case):
    def __init__(self, limit=0, two_d=False, host=False):
        self.limit, self.two_d, self.host = limit, two_d, host

    def inputs(self, seed):
        return [W.heights('levels8', SHAPE, seed=60 + seed), W.seeds('scattered', SHAPE, seed=70 + seed)]

    def call(self, args, sh):
        return rag.seeded_watershed(args[0], args[1], size_filter=self.limit, two_d=self.two_d, stream=sh)

    def read(self, result):
        labels, info = result
        return (labels if self.host else labels.cpu().numpy().view(np.uint64)), info

    def check(self, got, true):
        want, info = W.oracle(true[0], true[1], self.limit, self.two_d)
        assert_array_equal(got[0], want)
        assert (got[1].max_id, got[1].n_zero, got[1].n_dropped) == info
        assert self.limit == 0 or info[2] > 0


@pytest.mark.parametrize('case', [Watershed(), Watershed(limit=12), Watershed(limit=6, two_d=True),
                                  Watershed(limit=12, host=True)],
                         ids=['plain', 'size_filter', 'two_d_size_filter', 'host'])
def test_seeded_watershed_stays_on_its_stream(side, case):
    protocol_a(case, side)
