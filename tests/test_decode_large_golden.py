"""The CPU oracle's NMS-free decode beyond 900 x 10 scores and 300 rows against the REFERENCE's own NMSFreeCoder
(tests/golden/make_golden_decode.py -> g6_decode_c26.npz: 900 x 26 scores, max_num 300 and 1000, with and without a
score threshold).  The fixture's scores are many ulps apart, so the selection is exact; tests/test_gpu_decode_stream.py
holds the streaming kernel to the same fixture.  No GPU."""
import os

import numpy as np
import pytest
import torch

from oracle import transcar_oracle as O


def fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g6_decode_c26.npz'))


def fixture_cases():
    return [(mx, name) for mx in (300, 1000) for name in ('none', 'thr')]


def test_fixture_scores_are_far_apart():
    """What the generator asserted, on the stored logits: neighbouring fp32 scores of the top 1 100 are >= 16 ulps apart."""
    g = fixture()
    assert g['cls'].shape == (1, 900, 26) and g['box'].shape == (1, 900, 10)
    s = np.sort(torch.from_numpy(g['cls']).double().sigmoid().float().numpy().reshape(-1))[::-1][:1100]
    assert np.diff(s[::-1].view(np.int32)).min() >= 16
    assert s[150] < float(g['score_threshold']) < s[149]


@pytest.mark.parametrize('max_num,name', fixture_cases())
def test_oracle_decode_matches_reference(max_num, name):
    g = fixture()
    thr = None if name == 'none' else float(g['score_threshold'])
    boxes, scores, labels = O.nms_free_decode(torch.from_numpy(g['cls'][0]), torch.from_numpy(g['box'][0]),
                                              [float(v) for v in g['post_center_range']], max_num=max_num,
                                              num_classes=26, score_threshold=thr)
    want_l = g['labels_%d_%s' % (max_num, name)]
    assert 0 < len(want_l) < max_num                     # the range mask (and the threshold) dropped rows
    np.testing.assert_array_equal(labels.numpy(), want_l)
    assert int(labels.max()) > 9                         # labels beyond ten classes
    np.testing.assert_allclose(scores.numpy(), g['scores_%d_%s' % (max_num, name)], atol=1e-6, rtol=0)
    np.testing.assert_allclose(boxes.numpy(), g['bboxes_%d_%s' % (max_num, name)], atol=2e-5, rtol=0)
    if thr is not None:
        assert float(scores.min()) > thr
