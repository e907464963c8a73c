"""The per-layer teacher-forced comparisons, shared by test_gpu_teacher_forced.py (the bench's rig)
and test_gpu_adverse_frame.py (the adverse rig of adverse_rig.py): ONE copy of the assertions and
of their constants, so that a rig cannot quietly be held to a looser standard than the other.

A ``rig`` is a dict with ``sd`` / ``sd64`` (the oracle's fp32 state dict and its .double() copy),
``head`` (the HIP head with the same weights, on the device), ``feats`` (host NCHW maps), ``nhwc``
(the same maps channels-last on the device), ``l2i`` [1,N,4,4] and the fp32 oracle's trace of the
decoder: ``hs`` [L,Q,1,C], ``init_ref``, ``inter_refs``.  ``pcr`` / ``hw``: the rig's point-cloud range and image
size where they are not the configs' (rig_pcr, rig_hw).

Reference lines: XFMR:178-214 (decoder loop + refinement), XFMR:346-378 (cross attention),
HEAD:538-729 (three fusion layers)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import transcar_oracle as O
from transcar_amd import configs
from transcar_amd.detr3d_head import MATRIX_PATHS

# the configs' range and image size, for the rigs that name them; the checks read the rig's (rig_pcr, rig_hw)
PCR = configs.point_cloud_range
HW = configs.IMG_SHAPE[:2]
# One layer on identical inputs; activations are LayerNorm outputs, |x| up to ~5.  On these
# un-conditioned inputs the fp32 REFERENCE formula itself deviates from its fp64 evaluation by up to
# 1.6e-4 per layer (max over 900 x 256 values; mean 4e-6 -- measured, and re-measured by the test):
# iid-noise maps turn the fp32 rounding of a projected pixel coordinate (1e-4 px at |u| ~ 1600)
# into an O(1e-4) change of the sampled feature.  So the test measures both implementations against
# the fp64 evaluation ("truth") and asserts that HIP is as close to it as the fp32 oracle is.
LAYER_MAX_TOL = 3e-4      # max |hip - fp64| (the fp32 oracle reaches 1.6e-4)
LAYER_MEAN_TOL = 1e-5     # mean |hip - fp64| (the fp32 oracle: 4e-6)
LAYER_TOL = 1e-4          # radar layers (no sampling: plain linear algebra on O(1) values)
REF_TOL = 3e-5            # refined reference points (sigmoid of a full-xavier-scale MLP output; the fp32 oracle: 1.2e-5)


def rig_pcr(rig):
    return list(rig.get('pcr', configs.point_cloud_range))


def rig_hw(rig):
    return tuple(rig.get('hw', configs.IMG_SHAPE[:2]))


def dev():
    return torch.device('cuda:0')


def gpu(x):
    return torch.as_tensor(x).float().contiguous().to(dev())


def head_ops():
    from transcar_amd import ops
    return ops


def qkv_from_oracle_state(sd, lid, x, pos):
    """q (pre-scaled for the 2^x softmax), k, v^T of decoder layer `lid` from the oracle's layer
    input, computed on the host in fp64 and rounded once: the attention core's operands without
    any HIP arithmetic in front of it."""
    name = 'transformer.decoder.layers.%d.attentions.0.attn' % lid
    W, b = sd[name + '.in_proj_weight'].double(), sd[name + '.in_proj_bias'].double()
    C = 256
    qk_in = (x + pos).double()
    q = F.linear(qk_in, W[:C], b[:C]) * (1.4426950408889634 / np.sqrt(32.0))
    k = F.linear(qk_in, W[C:2 * C], b[C:2 * C])
    v = F.linear(x.double(), W[2 * C:], b[2 * C:])
    Q = x.shape[1]
    qpad = ((Q + 15) // 16) * 16
    vt = torch.zeros((x.shape[0], C, qpad), dtype=torch.float64)
    vt[:, :, :Q] = v.permute(0, 2, 1)
    return q.float(), k.float(), vt.float()


def decoder_layer_truth(rig, lid):
    """The fp64 evaluation of decoder layer `lid` on the fp32 oracle's layer-(lid-1) state: (hs
    [1,Q,C], refined reference points [1,Q,3]).  A function of the rig alone: kept in the rig, so
    the parametrised cases of one module evaluate it once."""
    cache = rig.setdefault('_decoder_truth', {})
    if lid not in cache:
        sd, sd64 = rig['sd'], rig['sd64']
        qe = sd['query_embedding.weight']
        pos = qe[:, :256][None]
        if '_feats64' not in rig:
            rig['_feats64'] = [f.double() for f in rig['feats']]
        x_prev = qe[:, 256:][None] if lid == 0 else rig['hs'][lid - 1].permute(1, 0, 2)
        ref_prev = rig['init_ref'] if lid == 0 else rig['inter_refs'][lid - 1]
        p = 'transformer.decoder.layers.%d.' % lid
        truth = O.decoder_layer(sd64, p, x_prev.permute(1, 0, 2).double(), pos.permute(1, 0, 2).double(),
                                rig['_feats64'], ref_prev.double(), rig_pcr(rig), rig['l2i'].double(), rig_hw(rig),
                                num_cams=rig['head'].weights_struct().num_cams).permute(1, 0, 2)
        tmp64 = O.reg_branch(sd64, 'reg_branches.%d' % lid, truth)
        new_ref = torch.zeros_like(ref_prev.double())
        new_ref[..., :2] = tmp64[..., :2] + O.inverse_sigmoid(ref_prev.double()[..., :2])
        new_ref[..., 2:3] = tmp64[..., 4:5] + O.inverse_sigmoid(ref_prev.double()[..., 2:3])
        cache[lid] = (truth, new_ref.sigmoid())
    return cache[lid]


def decoder_layers_teacher_forced(rig, tile_rows, matrix, title):
    """HIP layer l (attention core + fused row chain) on the oracle's layer-(l-1) state and
    reference points, l = 0..5 -- measured against the fp64 evaluation of the reference formula on
    the same inputs, next to the fp32 oracle's own deviation from it.  Also: the refined reference
    points and the next layer's projected q / k / v^T the chain hands to the following attention
    core.  Prints and returns the per-layer report."""
    ops = head_ops()
    sd, head = rig['sd'], rig['head']
    qe = sd['query_embedding.weight']
    pos = qe[:, :256][None]                                   # [1,Q,C]
    l2i = gpu(rig['l2i'])
    pv = head._packed_view
    w = head.weights_struct()          # the C layer struct carries neither the camera count nor the FFN's width
    L = 6
    report = []
    for lid in range(L):
        x_prev = qe[:, 256:][None] if lid == 0 else rig['hs'][lid - 1].permute(1, 0, 2)   # [1,Q,C]
        ref_prev = rig['init_ref'] if lid == 0 else rig['inter_refs'][lid - 1]
        q, k, vt = qkv_from_oracle_state(sd, lid, x_prev, pos)
        attn_o = ops.sdpa(gpu(q), gpu(k), gpu(vt), matrix_path='f16x2' if matrix == 'f16x2' else 'f32')
        nxt = pv.layers[lid + 1].self_attn.in_proj if lid + 1 < L else None
        hs, ref_out, qk_next, vt_next = ops.decoder_layer_tail(
            pv.layers[lid], nxt, rig['nhwc'], attn_o, gpu(x_prev), gpu(qe), l2i, gpu(ref_prev), rig_pcr(rig), rig_hw(rig),
            num_cams=w.num_cams, tile_rows=tile_rows, matrix_path=MATRIX_PATHS[matrix], ffn_dims=w.ffn_dims)
        # the same layer: fp32 oracle (from the rig's trace) and fp64 evaluation of the same formula
        truth, truth_ref = decoder_layer_truth(rig, lid)
        oracle32 = rig['hs'][lid].permute(1, 0, 2)            # [1,Q,C]
        e_hip = (hs.cpu().double() - truth).abs()
        e_o32 = (oracle32.double() - truth).abs()
        e_ref_hip = (ref_out.cpu().double() - truth_ref).abs()
        e_ref_o32 = (rig['inter_refs'][lid].double() - truth_ref).abs()
        # a query whose projected point sits within fp32 rounding of an image border / depth
        # threshold may flip its visibility mask (a discontinuity of the reference, XFMR:399-409):
        # allow <= 2 such rows per layer, everything else must hold the tolerance
        bad = (e_hip.amax(-1) > LAYER_MAX_TOL)[0]
        report.append('layer %d: max|hs - fp64| hip %.2e / fp32 oracle %.2e; mean %.2e / %.2e; '
                      'max|ref - fp64| %.1e / %.1e; rows over %.0e: %s' % (
                          lid, e_hip.max(), e_o32.max(), e_hip.mean(), e_o32.mean(), e_ref_hip.max(),
                          e_ref_o32.max(), LAYER_MAX_TOL, torch.where(bad)[0].tolist()[:16]))
        assert int(bad.sum()) <= 2, report[-1]
        ok = ~bad
        assert float(e_hip[0][ok].mean()) <= LAYER_MEAN_TOL, report[-1]
        # as close to the fp64 truth as the fp32 reference formula is (same order of magnitude)
        assert float(e_hip[0][ok].mean()) <= 2.0 * float(e_o32.mean()) + 1e-6, report[-1]
        assert float(e_hip[0][ok].max()) <= 2.0 * float(e_o32.max()) + 5e-5, report[-1]
        assert float(e_ref_hip[0][ok].max()) <= min(REF_TOL, 2.0 * float(e_ref_o32.max()) + 1e-6), report[-1]
        if nxt is not None:
            # the chain's projection of ITS hs for the next attention core, against the host
            # (fp64, rounded once) projection of the SAME hs
            q2, k2, vt2 = qkv_from_oracle_state(sd, lid + 1, hs.cpu(), pos)
            got_q, got_k = qk_next[..., :256].cpu(), qk_next[..., 256:].cpu()
            assert float((got_q - q2).abs().max()) <= 2e-5, lid
            assert float((got_k - k2).abs().max()) <= 2e-5, lid
            Q = hs.shape[1]
            assert float((vt_next.cpu()[0, :, :Q] - vt2[0, :, :Q]).abs().max()) <= 2e-5, lid
    print('\n'.join(['%s, tile_rows=%s matrix=%s:' % (title, tile_rows, matrix)] + report))
    return report


def hit_aware(got, want, got_hits, want_hits, tol, what):
    """compare rows whose gate decision agrees; bound the number of disagreeing rows"""
    agree = (got_hits == want_hits)
    assert int((~agree).sum()) <= 2, '%s: gate decisions differ on %d queries' % (what, int((~agree).sum()))
    d = np.abs(got - want)[agree]
    assert d.max() <= tol, '%s: max|d| = %.3g' % (what, d.max())
    return agree


def radar_layers_teacher_forced(rig, f36, tok_np, pad_mult, tile_rows, matrix, trace, min_hit_pairs=300):
    """The fused radar chain on one radar frame: all three layers in one launch from the oracle's
    hs[5] (the launch tc_head_forward makes), then ONE fusion layer at a time -- layer r is fed the
    oracle's query features and box of layer r-1 (hs[5] / the decoder's last box for r = 0) and must
    reproduce the oracle's class scores, boxes and hit counts of layer r.

    f36: the frame's feature rows as the oracle takes them; tok_np / pad_mult: the same frame as the
    HIP path takes it (radar.pack_tokens); trace: the oracle's (outputs, debug) of head_forward on
    f36.  Returns the one launch's (cls, box, hits) and the oracle's hit counts [3,Q]."""
    ops = head_ops()
    sd, head = rig['sd'], rig['head']
    want, dbg = trace
    want_cls = want['all_cls_scores'][:, 0].numpy()
    want_box = want['all_bbox_preds'][:, 0].numpy()
    want_hits = np.stack([h.numpy() for h in dbg['hit_counts']])
    assert want_hits.astype(bool).sum() > min_hit_pairs, 'the rig must exercise the gated attention'
    tokens = gpu(tok_np)
    hs5 = gpu(dbg['hs'][-1])                                  # [1,Q,C]
    ref5 = gpu(dbg['inter_refs'][-1])
    tmp = gpu(dbg['tmp'])                                     # the decoder's last box, metres
    # -- all three layers in one launch (what tc_head_forward does), from the oracle's decoder state
    from transcar_amd.detr3d_head import head_options
    opt = head_options(tile_rows=tile_rows or None, matrix_path=matrix)
    cls, box, hits = ops.radar_fusion(head, hs5, ref5, tmp, tokens, pad_mult, 0, 3, options=opt)
    agree0 = hit_aware(box[0, 0].cpu().numpy(), want_box[0], hits[0, 0].cpu().numpy(), want_hits[0],
                       LAYER_TOL, 'fusion layer 1 box')
    hit_aware(cls[0, 0].cpu().numpy(), want_cls[0], hits[0, 0].cpu().numpy(), want_hits[0],
              LAYER_TOL, 'fusion layer 1 cls')
    # fusion layers 2 and 3 of the SAME launch: layer r gates on layer r-1's own box, so a
    # query is compared once its gate decisions agree in every layer so far (a flipped gate changes the query's
    # later inputs); at most 2 new disagreements per layer, the layer-wise tolerance accumulates
    agree_all = agree0.copy()
    for r in (1, 2):
        now = hits[r, 0].cpu().numpy() == want_hits[r]
        assert int((agree_all & ~now).sum()) <= 2, 'fusion layer %d: %d new gate disagreements' % (r + 1, int((agree_all & ~now).sum()))
        agree_all &= now
        for name, got_, want_ in (('box', box[r, 0], want_box[r]), ('cls', cls[r, 0], want_cls[r])):
            d = np.abs(got_.cpu().numpy() - want_)[agree_all]
            assert d.max() <= LAYER_TOL * (r + 1), 'one launch, fusion layer %d %s: max|d| = %.3g' % (r + 1, name, d.max())
    assert int(agree_all.sum()) >= want_hits.shape[1] - 6
    # -- one layer at a time, teacher-forced.  Layer r's query features are not an output of the
    # head; recompute them with the oracle's layer function from its own previous state.
    qf = dbg['hs'][-1].permute(1, 0, 2)                       # [Q,1,C]
    radar_feat = dbg['radar_feat']
    tokens_full, _ = O.radar_tokens_from_features(f36)
    prev_box = dbg['tmp']
    for r, (sa, sf, rmin, rmax) in enumerate((('', '', 1.0, 2.0), ('2', '_2', 1.0, 2.0), ('3', '_3', 0.5, 1.0))):
        if r == 0:
            ref, PCR = dbg['inter_refs'][-1], rig_pcr(rig)
            cxy = torch.stack([ref[..., 0] * (PCR[3] - PCR[0]) + PCR[0],
                               ref[..., 1] * (PCR[4] - PCR[1]) + PCR[1]], -1)
        else:
            cxy = prev_box[..., :2]
        mask = O.circle_mask(cxy, prev_box[..., 3], prev_box[..., 6], prev_box[..., 7],
                             tokens_full[:, :, :2], rmin, rmax)
        cls_r, box_r, hits_r = ops.radar_fusion(head, gpu(qf.permute(1, 0, 2)),
                                                ref5 if r == 0 else None, gpu(prev_box), tokens,
                                                pad_mult, r, 1, options=opt)
        hit_aware(box_r[r, 0].cpu().numpy(), want_box[r], hits_r[r, 0].cpu().numpy(),
                  want_hits[r], LAYER_TOL, 'fusion layer %d box (teacher-forced)' % (r + 1))
        hit_aware(cls_r[r, 0].cpu().numpy(), want_cls[r], hits_r[r, 0].cpu().numpy(), want_hits[r],
                  LAYER_TOL, 'fusion layer %d cls (teacher-forced)' % (r + 1))
        assert torch.isnan(cls_r[(r + 1) % 3]).all()          # only the requested layer was written
        qf, _ = O.radar_layer(sd, sa, sf, qf, radar_feat, mask)
        prev_box = want['all_bbox_preds'][r]
    return (cls, box, hits), want_hits
