"""Decoder layer 0 from its pack-time constants (chain.hip PROG_DECODER_L0_T): in an eval-mode tc_head_forward the
layer's out_proj, norm0 and pe.3 are not run -- their results on the Q query rows were made once per checkpoint and
per kernel variant by that variant's own kernels.  The yardstick is bit-identity: layer 0 of the forward against the
SAME layer through the unchanged tc_decoder_layer_tail_fwd (always the full chain) at the same tile height and matrix
path, fed the packed view's l0_attn_out / l0_init_reference and the query embedding.  pytest -m gpu"""
import numpy as np
import pytest
import torch

from head_variant_rig import (HW, PCR, SMOOTH, TINY, T, dev, gpu, no_grad,  # noqa: F401  (T, no_grad: fixtures)
                              shared_head)
from transcar_amd import synth

pytestmark = pytest.mark.gpu

MATRIX = {None: 0, 'f32': 1, 'f16x2': 2}          # TC_MATRIX_*

# every (tile height, matrix path) tc_head_forward selects a row-chain kernel variant by, and the automatic choice
VARIANTS = [(4, 'f32'), (8, 'f32'), (16, 'f32'), (16, 'f16x2'), (32, 'f16x2'), (None, None)]


def make_head(T, **variant):
    return shared_head(T, **variant)[0]


def _inputs(head, B, nl=4):
    """B different frames: NHWC levels, lidar2img, radar tokens."""
    from transcar_amd import ops
    shapes = TINY[:nl]
    feats = [synth.make_feats(shapes, seed=40 + i, smooth=SMOOTH) for i in range(B)]
    frames = [synth.make_radar_frame(seed=60 + i, n_per_radar=45) for i in range(B)]
    metas = synth.make_img_metas(B, synth.make_lidar2img(), radar=frames if B > 1 else frames[0])
    nhwc = ops.to_nhwc_levels([gpu(np.concatenate([f[l] for f in feats], 0)) for l in range(nl)])
    tokens, pad_mult = head.radar_tokens(metas, dev())
    return nhwc, ops.lidar2img_tensor(metas, dev()), tokens, pad_mult


def _forward(head, inp, rows, matrix, **opts):
    from transcar_amd.detr3d_head import head_options
    nhwc, l2i, tokens, pad_mult = inp
    o = head.forward_nhwc(nhwc, l2i, HW, tokens, pad_mult, aux=True,
                          options=head_options(tile_rows=rows, matrix_path=matrix, **opts))
    torch.cuda.synchronize()
    return o


def _packed_tensor(head, ptr, shape):
    """A [..] fp32 tensor over the packed buffer at device address `ptr`."""
    off = int(ptr) - head._packed.data_ptr()
    n = int(np.prod(shape)) * 4
    assert 0 <= off and off + n <= head._packed.numel() * head._packed.element_size()
    return head._packed.view(torch.uint8)[off:off + n].view(torch.float32).view(*shape)


def _layer0_by_the_full_chain(head, inp, B, rows, matrix):
    from transcar_amd import ops
    head.head_weights()
    pv = head._packed_view
    Q = head.num_query
    attn_o = _packed_tensor(head, pv.l0_attn_out, (Q, 256))
    init_ref = _packed_tensor(head, pv.l0_init_reference, (Q, 3))
    qe = head.query_embedding.weight
    nhwc, l2i = inp[0], inp[1]
    hs, ref_out, _, _ = ops.decoder_layer_tail(
        pv.layers[0], pv.layers[1].self_attn.in_proj, nhwc, attn_o[None].expand(B, Q, 256).contiguous(),
        qe[:, 256:][None].expand(B, Q, 256).contiguous(), qe, l2i, init_ref[None].expand(B, Q, 3).contiguous(), PCR, HW,
        tile_rows=rows or 0, matrix_path=MATRIX[matrix])
    torch.cuda.synchronize()
    return hs, ref_out, init_ref


@pytest.mark.parametrize('B', [1, 2, 9])
@pytest.mark.parametrize('rows,matrix', VARIANTS)
def test_layer0_of_the_forward_is_the_full_chain_bit_for_bit(T, rows, matrix, B):
    head = make_head(T)
    inp = _inputs(head, B)
    aux = _forward(head, inp, rows, matrix)['aux']
    hs, ref_out, _ = _layer0_by_the_full_chain(head, inp, B, rows, matrix)
    assert torch.isfinite(hs).all() and float(hs.abs().max()) > 0.1
    assert torch.equal(aux['inter_states'][0], hs)
    assert torch.equal(aux['inter_references'][0], ref_out)


@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (16, 'f16x2'), (32, 'f16x2')])
def test_layer0_without_box_refinement(T, rows, matrix):
    """with_box_refine=False at one point and four levels takes the folded sequence too (no reg branch: K_NOP steps)."""
    head = make_head(T, with_box_refine=False)
    inp = _inputs(head, 2)
    aux = _forward(head, inp, rows, matrix)['aux']
    hs, ref_out, init_ref = _layer0_by_the_full_chain(head, inp, 2, rows, matrix)
    assert torch.equal(aux['inter_states'][0], hs)
    assert torch.equal(ref_out[0], init_ref)                       # (the layer op without a reg branch: ref_out = ref_in)
    assert torch.equal(aux['inter_references'][0], ref_out)


@pytest.mark.parametrize('kw', [dict(num_points=5), dict(num_levels=2)], ids=['num_points5', 'num_levels2'])
@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (32, 'f16x2')])
def test_generic_heads_keep_the_full_chain(T, kw, rows, matrix):
    """num_points > 1 and fewer than four levels run the generic kernels, whose layer 0 keeps today's chain (the layer
    op does not take such heads, so no comparison with it): the forward works from a packed buffer without the constants,
    and a frame's rows do not depend on the frames beside it (layer 0 reads its constants row % Q)."""
    head = make_head(T, **kw)
    nl = kw.get('num_levels', 4)
    two = _inputs(head, 2, nl)
    one = _inputs(head, 1, nl)
    a2 = _forward(head, two, rows, matrix)['aux']
    a1 = _forward(head, one, rows, matrix)['aux']
    assert torch.isfinite(a2['inter_states']).all()
    assert torch.equal(a2['inter_states'][:, 0], a1['inter_states'][:, 0])
    assert torch.equal(a2['inter_references'][:, 0], a1['inter_references'][:, 0])


def test_constants_are_those_of_the_selected_variant(T):
    """The variants' constants differ in their last bits (fp32 FMA chains against two-plane f16 products), which is why
    there is a block per variant; 5e-4 is test_gpu_training's bound between the two matrix paths' decoder states."""
    head = make_head(T)
    nine = _inputs(head, 9)
    a32 = _forward(head, nine, 32, 'f16x2')['aux']
    a16 = _forward(head, nine, 16, 'f32')['aux']
    d = float((a32['inter_states'][0] - a16['inter_states'][0]).abs().max())
    assert 0.0 < d < 5e-4, d


def test_packed_buffer_holds_the_constants_inside_its_size(T):
    """tc_head_packed_bytes covers the constants: the last variant's block ends inside the buffer, and every block holds
    finite values whose second tensor is the first + query_pos."""
    import ctypes
    from transcar_amd import _lib as L
    head = make_head(T)
    head.head_weights()
    Q = head.num_query
    nbytes = L.lib().tc_head_packed_bytes(ctypes.byref(head._weights))
    assert nbytes == head._packed.numel() * head._packed.element_size()
    plane = ((Q * 256 * 4 + 255) // 256) * 256
    first = int(head._packed_view.l0_attn_out) + plane - head._packed.data_ptr()
    assert first + 5 * 3 * plane <= nbytes
    blocks = head._packed.view(torch.uint8)[first:first + 5 * 3 * plane].view(torch.float32).view(5, 3, plane // 4)[:, :, :Q * 256]
    assert torch.isfinite(blocks).all()
    qe = head.query_embedding.weight
    for v in range(5):                              # norm0's second output is the first + query_pos
        assert torch.equal(blocks[v, 1].view(Q, 256), blocks[v, 0].view(Q, 256) + qe[:, :256])
    assert not torch.equal(blocks[0], blocks[4])    # 4-row fp32 against 32-row f16x2


def test_train_mode_decoder_is_not_folded_and_keeps_its_reference_check(T):
    """decoder_dropout_p > 0: layer 0 runs its whole chain behind the prologue and the attention core, as before --
    the existing check against the reference formula with the same masks, unchanged."""
    import test_gpu_training as TG
    from conftest import GOLDEN
    from transcar_amd import autograd_ops
    TG.test_decoder_train_mode_dropout_matches_reference_formula(autograd_ops, GOLDEN)
