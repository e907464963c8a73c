#!/usr/bin/env python3
"""The box decode beyond 900 x 10 scores and 300 rows, from the REFERENCE's own NMSFreeCoder (oracle/ref_harness.py).
Run only in the authoring container:
    python tests/golden/make_golden_decode.py

  g6_decode_c26.npz    seeded logits [1, 900, 26] and box codes [1, 900, 10], and what
                       NMSFreeCoder(num_classes=26).decode_single returns from them for max_num 300 and 1000, without a
                       score threshold and with one inside the score range

The logits are a seeded permutation of a grid, np.linspace(-8, 4, 23 400): the fp32 sigmoids of the top 1 100 are many
ulps apart from their neighbours (asserted below), so which (query, class) pairs are selected, and in which order, is
no matter of anyone's rounding.  A fifth of the centres lie outside post_center_range: the range mask has work to do."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG                                 # noqa: E402

Q, NCLS, CODE = 900, 26, 10
MAX_NUMS = (300, 1000)
MIN_ULPS = 16          # between neighbouring fp32 scores of the top 1 100


def decode_inputs(seed=26):
    rng = np.random.RandomState(seed)
    n = Q * NCLS
    cls = np.linspace(-8.0, 4.0, n).astype(np.float32)[rng.permutation(n)].reshape(1, Q, NCLS)
    box = (rng.standard_normal((1, Q, CODE)) * 0.3).astype(np.float32)
    box[..., 0] *= 150.0           # cx, cy: sigma 45 m against +-61.2
    box[..., 1] *= 150.0
    box[..., 4] *= 15.0            # cz: sigma 4.5 m against +-10
    return cls, box


def main():
    ref = MG.RH.load_reference()
    cfg = {k: v for k, v in MG.configs.pts_bbox_head['bbox_coder'].items() if k != 'type'}
    cls, box = decode_inputs()
    top = np.sort(torch.from_numpy(cls).double().sigmoid().float().numpy().reshape(-1))[::-1][:1100]
    gaps = np.diff(top[::-1].view(np.int32))               # positive floats: the bit patterns count ulps
    assert gaps.min() >= MIN_ULPS, gaps.min()
    thr = float(np.float32((np.float64(top[149]) + np.float64(top[150])) * 0.5))      # keeps 150 of the selected rows
    assert top[150] < thr < top[149]
    arrs = dict(cls=cls, box=box, score_threshold=np.float32(thr), post_center_range=np.asarray(cfg['post_center_range'], np.float32))
    for mx in MAX_NUMS:
        for name, t in (('none', None), ('thr', thr)):
            coder = ref.CODER.NMSFreeCoder(**dict(cfg, max_num=mx, num_classes=NCLS, score_threshold=t))
            out = coder.decode_single(torch.from_numpy(cls[0]), torch.from_numpy(box[0]))
            n_kept = out['scores'].shape[0]
            assert 0 < n_kept < (mx if t is None else 150), (mx, name, n_kept)      # the range mask dropped some
            for k in ('bboxes', 'scores', 'labels'):
                arrs['%s_%d_%s' % (k, mx, name)] = out[k].numpy()
    MG.save('g6_decode_c26.npz', **arrs)


if __name__ == '__main__':
    main()
