"""Host-side mirror of the reference's
projects/mmdet3d_plugin/models/dense_heads/detr3d_head.py (HEAD:33-1023):
``Detr3DHead`` with the reference's ctor kwargs (the ``pts_bbox_head`` config
block, CFG:51-102), forward signature, output dict and state_dict keys.

``forward`` is ONE call into the HIP library (tc_head_forward): 6 decoder
layers + radar encoders + 3 distance-gated radar fusion layers, fp32, eval
mode.  Differences to the reference that are part of the contract:
  * radar arrives through ``img_metas[i]['radar']`` (raw sweeps or [n,36]
    features) instead of a nuScenes devkit lookup on ``sample_idx`` with disk
    reads inside forward (HEAD:27, 301-309);
  * the six cls branches / five of six reg branches whose results the
    reference computes and throws away (HEAD:277-298, lists reset at
    HEAD:607-608) are not evaluated by the default ``outputs='fusion'``;
    ``outputs='camera'`` / ``'all'`` return them (tc_decoder_outputs_fwd);
  * with_box_refine=False (one shared cls / reg branch, HEAD:223-231): the
    decoder samples every layer at the initial reference points and runs no
    reg branch below its last layer (tc_decoder_layer.reg);
  * batch size > 1 is supported for the radar part too (the reference
    hard-codes B = 1: HEAD:301, 523, 568).
There is no CPU fallback.
"""
import copy
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib as L
from . import ops, radar
from .bricks import BaseModule, mha_view, require_eval
from .detr3d_transformer import pos_encoder_view
from . import hungarian_assigner_3d, losses                  # noqa: F401 (registers)
from .bbox_util import normalize_bbox
from .registry import (BBOX_ASSIGNERS, HEADS, build_bbox_coder,
                       build_transformer)

RADAR_RADII = L.RADAR_RADII                            # HEAD:567, 635, 693: the default of Detr3DHead(radar_gate=)
OUTPUTS = ('fusion', 'camera', 'all')                  # Detr3DHead.outputs


def _env_tile_rows():
    """TRANSCAR_CHAIN_ROWS (host-side tuning knob, read once at import, validated)."""
    import os
    v = os.environ.get('TRANSCAR_CHAIN_ROWS', '0')
    if v not in ('0', '4', '8', '16', '32'):
        raise ValueError('TRANSCAR_CHAIN_ROWS=%r (0 = automatic, 4, 8, 16 or 32)' % v)
    return int(v)


DEFAULT_TILE_ROWS = _env_tile_rows()


MATRIX_PATHS = {None: L.TC_MATRIX_AUTO, 'auto': L.TC_MATRIX_AUTO, 'f32': L.TC_MATRIX_F32, 'f16x2': L.TC_MATRIX_F16X2}


def head_options(tile_rows=None, unfused=None, last_level_cls_only=False,
                 decoder_dropout_p=0.0, dropout_seed=0, radar_compact=None, phase=0, matrix_path=None,
                 dropout_seed_stride=0, cam_pregather=None):
    """tc_head_options for one forward.  unfused=None: the TRANSCAR_UNFUSED=1
    environment switch of the operator-by-operator cross-check path (a host-side
    knob: the library itself reads no environment)."""
    import os
    o = L.tc_head_options()
    o.chain_tile_rows = int(tile_rows) if tile_rows else DEFAULT_TILE_ROWS
    o.unfused = int(os.environ.get('TRANSCAR_UNFUSED', '0') == '1') if unfused is None else int(bool(unfused))
    o.last_level_cls_only = int(bool(last_level_cls_only))
    o.decoder_dropout_p = float(decoder_dropout_p)
    # radar_compact: None = automatic (beyond one frame per launch), False / True = never / always
    o.radar_row_order = 0 if radar_compact is None else (2 if radar_compact else 1)
    o.dropout_seed = int(dropout_seed) & 0xFFFFFFFFFFFFFFFF
    o.phase = int(phase)          # 0: the whole forward; 1 / 2: before / after the radar tokens exist (forward_nhwc)
    # 16-row tiles: 'f16x2' (= automatic) two-plane f16 operands on the matrix cores, 'f32' the exact fp32 MFMA
    o.matrix_path = MATRIX_PATHS[matrix_path] if not isinstance(matrix_path, int) else int(matrix_path)
    # decoder dropout of a batch of frames: sample b draws the masks of seed + b * stride, indices relative to the sample
    o.dropout_seed_stride = int(dropout_seed_stride) & 0xFFFFFFFFFFFFFFFF
    # opt-in (ABI 12): the camera gather of a decoder layer as extra workgroups of the attention-core launch in front of
    # its chain (f16x2 launches); forward_nhwc supplies the scratch.  Bit-identical outputs; 1 % faster with one launch
    # sequence at a time, 2.8 % slower with three in flight: off by default
    o.cam_pregather = 1 if cam_pregather else 0
    return o


#: module-name suffixes of fusion layer 1, 2, 3: (rf_linear* / rf_norm* / rf_dropout*, rf_multihead_attn* / final_*)
FUSION_SUFFIXES = (('', ''), ('_2', '2'), ('_3', '3'))


def fusion_module_names(r):
    """field -> attribute name of fusion layer r's modules (0-based; HEAD:129-171): the one place that knows the suffixes."""
    sfx, asfx = FUSION_SUFFIXES[r]
    names = dict(attn='rf_multihead_attn' + asfx, linear1='rf_linear1' + sfx, linear2='rf_linear2' + sfx,
                 final_cls='final_cls' + asfx, final_reg='final_reg' + asfx, dropout='rf_dropout' + sfx)
    for n in (1, 2, 3):
        names['norm%d' % n] = 'rf_norm%d%s' % (n, sfx)
        names['dropout%d' % n] = 'rf_dropout%d%s' % (n, sfx)
    return names


def fusion_modules(head, r):
    """The modules of fusion layer r of `head` under their field names (``.attn``, ``.norm2``, ``.final_cls``, ...)."""
    return SimpleNamespace(**{field: getattr(head, name) for field, name in fusion_module_names(r).items()})


#: coefficient of the forward counter in `dropout_seed_of`: consecutive training forwards draw seeds this far apart
SEED_STRIDE = 0x85EBCA77


def dropout_seed_of(dropout_seed, rank, n):
    """Seed of the counter-based dropout masks of a process's n-th training forward (n = 1 for the first)."""
    return (int(dropout_seed) * 0x9E3779B1 + rank * 0xC2B2AE3D27D4EB4F + n * SEED_STRIDE + 1) & 0xFFFFFFFFFFFFFFFF


def _rank():
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def radar_frames(img_metas):
    """[img_metas[i]['radar']]; a frame without one is refused."""
    if any('radar' not in m for m in img_metas):
        raise KeyError("img_metas[i]['radar'] is required: raw sweeps (transcar_amd/radar.py) or an [n,radar_in_dims] feature array")
    return [m['radar'] for m in img_metas]


def _cls_branch(embed, ncls):
    return nn.Sequential(
        nn.Linear(embed, embed), nn.LayerNorm(embed), nn.ReLU(inplace=True),
        nn.Linear(embed, embed), nn.LayerNorm(embed), nn.ReLU(inplace=True),
        nn.Linear(embed, ncls))


def _reg_branch(embed, code, inplace=True):
    return nn.Sequential(
        nn.Linear(embed, embed), nn.ReLU(inplace=inplace),
        nn.Linear(embed, embed), nn.ReLU(inplace=inplace),
        nn.Linear(embed, code))


def _lin(m, ptr=ops._p):
    return L.tc_linear(ptr(m.weight), ptr(m.bias))


def _ln(m, ptr=ops._p):
    return L.tc_lnorm(ptr(m.weight), ptr(m.bias))


def cls_branch_view(seq, ptr=ops._p):
    return L.tc_cls_branch(_lin(seq[0], ptr), _ln(seq[1], ptr), _lin(seq[3], ptr), _ln(seq[4], ptr), _lin(seq[6], ptr))


def reg_branch_view(seq, ptr=ops._p):
    return L.tc_reg_branch(_lin(seq[0], ptr), _lin(seq[2], ptr), _lin(seq[4], ptr))


def radar_table(head, w, ptr=ops._p):
    """Fill the radar stack's part of the tc_head_weights `w` (the two encoders, ``head.num_fusion_layers`` layers) with
    ptr(tensor): the parameters' addresses (Detr3DHead.weights_struct) or their gradients' (trainer.grad_table)."""
    rpe, rfe = head.radar_position_encoder, head.radar_feat_encoder
    w.radar_position_encoder = L.tc_pos_encoder(_lin(rpe[0], ptr), _ln(rpe[1], ptr), _lin(rpe[3], ptr), _ln(rpe[4], ptr))
    w.radar_feat0, w.radar_feat2, w.radar_feat4 = _lin(rfe[0], ptr), _lin(rfe[2], ptr), _lin(rfe[4], ptr)
    w.num_radar_layers = L.check_num_fusion_layers(head.num_fusion_layers)
    for r in range(w.num_radar_layers):
        m, rl = fusion_modules(head, r), w.radar[r]
        rl.attn = L.tc_mha(L.tc_linear(ptr(m.attn.in_proj_weight), ptr(m.attn.in_proj_bias)), _lin(m.attn.out_proj, ptr))
        rl.norm2, rl.norm3 = _ln(m.norm2, ptr), _ln(m.norm3, ptr)
        rl.linear1, rl.linear2 = _lin(m.linear1, ptr), _lin(m.linear2, ptr)
        rl.final_cls, rl.final_reg = cls_branch_view(m.final_cls, ptr), reg_branch_view(m.final_reg, ptr)
    return w


@HEADS.register_module(export=True)
class Detr3DHead(BaseModule):
    """Head of Detr3D + the TransCAR radar fusion decoder."""

    def __init__(self, num_classes, in_channels, num_query=100, num_reg_fcs=2,
                 transformer=None, sync_cls_avg_factor=False,
                 positional_encoding=None, loss_cls=None, loss_bbox=None,
                 loss_iou=None, train_cfg=None, test_cfg=None, init_cfg=None,
                 with_box_refine=False, as_two_stage=False, bbox_coder=None,
                 num_cls_fcs=2, code_weights=None, outputs='fusion', num_fusion_layers=3, radar_gate=None,
                 radar_num_heads=L.TC_RADAR_HEADS, radar_num_tokens=L.TC_RADAR_TOKENS_REF,
                 radar_in_dims=L.RADAR_IN_DIMS_REF, radar_point_range=None, **kwargs):
        super().__init__(init_cfg)
        #: the radar input (_lib.check_radar_input).  radar_num_tokens N: a frame's first N kept points are attended, the
        #: rest dropped (HEAD:526-530 at 1500); pad_mult = N - T + 1.  radar_in_dims F: features per token, columns 0..2 being
        #: x, y, z -- radar_feat_encoder.0 is Linear(F, 64), so a checkpoint of another F fails to load by shape; with
        #: F != 36 raw sweeps are refused (their 36 features are the reference's) and frames arrive as [n,F] rows.
        #: radar_point_range: the radar filter's range, by default the reference's constant (HEAD:304) -- it does not
        #: follow pc_range.  Raw sweeps and [n,F] rows given as CUDA tensors are always filtered by it; [n,F] rows on the
        #: host (numpy, CPU tensors) are filtered by a range other than the default and taken as they are at the default
        #: (the reference's rows come out of its own filter).  Configuration: a trainer checkpoint records none of the three
        self.radar_num_tokens, self.radar_in_dims, self.radar_point_range = L.check_radar_input(
            radar_num_tokens, radar_in_dims, radar_point_range)
        #: depth N of the radar fusion stack, 1 .. 3 (the reference builds 3): only the first N sets of rf_* / final_*
        #: modules exist, every output has N fusion levels.  Level k reads layers <= k only, so an N-layer head with the
        #: first N layers' weights computes levels [0:N] of the three-layer head
        self.num_fusion_layers = L.check_num_fusion_layers(num_fusion_layers)
        #: the distance gate of the fusion layers, normalised (_lib.check_radar_gate): dict(type='three_circle', radii=
        #: ((rmin, rmax), ...)) -- the reference head's gate, RADAR_RADII by default -- or dict(type='circle', radii=(R, ...)),
        #: the single circle of the paper's radius ablation (a token attended iff not dist > R).  Configuration, like
        #: pc_range: it adds no parameter, so the weights of either kind of head load into the other unchanged
        self.radar_gate = L.check_radar_gate(radar_gate, self.num_fusion_layers)
        #: heads of the fusion attention rf_multihead_attn{,2,3}: 4, 8 (the reference's, HEAD:129-171) or 16, head dimension
        #: 64 / 32 / 16.  Configuration too: in_proj / out_proj keep their shapes, a checkpoint records nothing about it
        self.radar_num_heads = L.check_radar_num_heads(radar_num_heads)
        if outputs not in OUTPUTS:
            raise ValueError("Detr3DHead: outputs=%r (one of 'fusion', 'camera', 'all')" % (outputs,))
        #: what ``forward`` returns as all_cls_scores / all_bbox_preds: 'fusion' the radar fusion levels (three by default; the
        #: reference's return value), 'camera' the L decoder levels of the DETR3D camera detector alone (HEAD:277-298;
        #: radar is neither read nor required), 'all' the decoder levels followed by the fusion levels (the reference
        #: with HEAD:607-608 commented out).  A plain attribute: it may be changed between forwards.
        self.outputs = outputs
        if as_two_stage:
            raise NotImplementedError('as_two_stage is not used by TransCAR')
        self.with_box_refine = with_box_refine
        self.as_two_stage = as_two_stage
        self.code_size = kwargs.get('code_size', 10)
        code_weights = code_weights if code_weights is not None else \
            [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.pc_range = self.bbox_coder.pc_range
        self.num_cls_fcs = num_cls_fcs - 1
        # --- what mmdet's DETRHead.__init__ sets
        self.bg_cls_weight = 0
        self.sync_cls_avg_factor = sync_cls_avg_factor
        self.num_query = num_query
        self.num_classes = num_classes
        self.in_channels = in_channels
        self.num_reg_fcs = num_reg_fcs
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        self.fp16_enabled = False
        self.loss_cls_cfg = dict(loss_cls or {})
        self.loss_bbox_cfg = dict(loss_bbox or {})
        self.loss_iou_cfg = dict(loss_iou or {})
        use_sigmoid = self.loss_cls_cfg.get('use_sigmoid', False)
        self.cls_out_channels = num_classes if use_sigmoid else num_classes + 1
        self.transformer = build_transformer(transformer)
        self.embed_dims = self.transformer.embed_dims
        # The reference samples the cameras with Detr3DCrossAtten.pc_range (XFMR:366) and de-normalises the boxes with
        # the coder's; the fused path packs ONE range for both, so a config in which they differ is refused rather than
        # sampled with the coder's
        for name, m in self.transformer.named_modules():
            rng = getattr(m, 'pc_range', None)
            if rng is not None and [float(v) for v in rng] != [float(v) for v in self.pc_range]:
                raise ValueError('Detr3DHead: transformer.%s.pc_range %s differs from bbox_coder.pc_range %s; the fused '
                                 'kernels take one point-cloud range for the camera sampling and the boxes'
                                 % (name, list(rng), list(self.pc_range)))
        self.assigner = None
        if train_cfg and train_cfg.get('assigner') is not None:
            self.assigner = BBOX_ASSIGNERS.build(train_cfg['assigner'])
        self._init_layers()
        # --- HEAD:70-196
        self.code_weights = nn.Parameter(
            torch.tensor(code_weights, requires_grad=False),
            requires_grad=False)
        E, F = self.embed_dims, L.TC_RADAR_FFN_DIMS
        names = [fusion_module_names(r) for r in range(self.num_fusion_layers)]
        for nm in names:
            setattr(self, nm['final_cls'], _cls_branch(E, self.cls_out_channels))
            setattr(self, nm['final_reg'], _reg_branch(E, self.code_size))
        for nm in names:
            setattr(self, nm['attn'], nn.MultiheadAttention(E, self.radar_num_heads, dropout=0.1))
            setattr(self, nm['linear1'], nn.Linear(E, F))
            setattr(self, nm['linear2'], nn.Linear(F, E))
            for n in ('norm1', 'norm2', 'norm3'):
                setattr(self, nm[n], nn.LayerNorm(E))
            # HEAD:132, 138-140 (rf_dropout1* is constructed but never used there either)
            for n in ('dropout', 'dropout1', 'dropout2', 'dropout3'):
                setattr(self, nm[n], nn.Dropout(0.1))
        self.radar_position_encoder = nn.Sequential(
            nn.Linear(3, E), nn.LayerNorm(E), nn.ReLU(inplace=True),
            nn.Linear(E, E), nn.LayerNorm(E), nn.ReLU(inplace=True))
        self.radar_feat_encoder = nn.Sequential(
            nn.Linear(self.radar_in_dims, 64), nn.ReLU(inplace=True),
            nn.Linear(64, 128), nn.ReLU(inplace=True),
            nn.Linear(128, E), nn.ReLU(inplace=True))
        # constructed but never used by the reference forward (HEAD:191-195); kept at every fusion depth, so that the
        # reference's checkpoint minus the absent layers' keys loads strictly
        self.attention_weights2 = nn.Linear(E, 6 * 4)
        self.attention_weights3 = nn.Linear(E, 6 * 4)
        self.output_proj2 = nn.Linear(E, E)
        self.output_proj3 = nn.Linear(E, E)
        self._weights = None
        self._workspace = {}
        self._packed = None
        self._packed_view = None        # tc_head_weights over `_packed`, written by `_pack`
        #: the dropout masks of a training forward: seed base (FusionTrainer(seed=)), training forwards so far, last seed
        self.dropout_seed = 0
        self._train_forwards = 0
        self.last_dropout_seed = None
        #: cls_branches / reg_branches packed for tc_decoder_outputs_fwd: (buffer, view, key), built by the first
        #: forward with outputs != 'fusion', dropped whenever the packed weights are (refresh_weights, load_state_dict)
        self._dec_heads = None
        #: (buffer, bytes of the struct it was packed from) of the last `decoder_heads()` pack; outlives `_dec_heads`, so
        #: that the next pack writes the same buffer (dropped with the device: `_apply`)
        self._dec_heads_last = None
        #: the trainable (radar) weights changed in place since they were last re-packed
        #: (an optimizer step): the next forward / pipeline replay that reads them re-packs first
        self._packed_dirty = False
        #: 'device' (default): raw radar sweeps in img_metas are turned into tokens by tc_radar_build_tokens_batch;
        #: 'host': the reference's numpy route (transcar_amd/radar.py)
        self.radar_ingest = 'device'
        #: tc_head_options of ``forward`` (``head_options(...)``; None = defaults: automatic tile height and matrix path)
        self.forward_options = None
        #: f16-range guard (tc_head_options.range_status): word 0 of ``_status_buf`` is OR-ed with 1 by the f16x2 kernels
        #: when a linear step produces a non-finite value (an operand beyond the f16 planes' range turns into inf / NaN,
        #: never into a wrong finite number); get_bboxes reads it with the decode's counts and, on the automatic matrix
        #: path, switches this head to the exact-fp32 kernels (``matrix_fallback``) from the next forward on
        self._status_buf = None
        self.matrix_fallback = False
        self.matrix_fallback_generation = -1
        #: the plugin entry as cached hipGraphs (transcar_amd/plugin_graph.py); ``plugin_graphs = False``: always eager
        self._plugin_graphs = None
        self.plugin_graphs = True
        self._radar_stage = {}
        self._radar_range = None        # ((device, radar_point_range), the range as six float64 on the device)
        self._ingest_streams = {}       # device -> side stream of the two-phase forward (forward_nhwc(fill_tokens=))
        #: bumped whenever a device buffer a captured hipGraph may point at (packed weights,
        #: lane workspaces) is re-allocated: FramePipeline refuses to replay a stale capture
        self.buffers_generation = 0

    def _init_layers(self):
        """HEAD:198-238."""
        E = self.embed_dims
        num_pred = self.transformer.decoder.num_layers
        fc_cls = _cls_branch(E, self.cls_out_channels)
        reg_branch = _reg_branch(E, self.code_size, inplace=False)
        if self.with_box_refine:
            self.cls_branches = nn.ModuleList(
                [copy.deepcopy(fc_cls) for _ in range(num_pred)])
            self.reg_branches = nn.ModuleList(
                [copy.deepcopy(reg_branch) for _ in range(num_pred)])
        else:
            self.cls_branches = nn.ModuleList([fc_cls] * num_pred)
            self.reg_branches = nn.ModuleList([reg_branch] * num_pred)
        self.query_embedding = nn.Embedding(self.num_query, E * 2)

    def init_weights(self):
        """HEAD:240-246."""
        self.transformer.init_weights()
        if self.loss_cls_cfg.get('use_sigmoid', False):
            bias_init = float(-np.log((1 - 0.01) / 0.01))
            for m in self.cls_branches:
                nn.init.constant_(m[-1].bias, bias_init)

    # ------------------------------------------------------------------
    # parameter views for the C ABI
    # ------------------------------------------------------------------
    def _apply(self, fn, *a, **k):
        self._weights = None            # pointers move on .to()/.cuda()
        self._workspace = {}
        self._packed = None
        self._dec_heads = None
        self._dec_heads_last = None
        self.buffers_generation += 1
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._weights = None
        self._dec_heads = None
        return super().load_state_dict(*a, **k)

    def reload_state_dict(self, state_dict, strict=True):
        """``load_state_dict`` into a head whose packed weights captured hipGraphs may point at (FusionTrainer.
        load_checkpoint): torch copies the values into the parameters where they lie, the packed copies are written again
        at once and in place, and ``refresh_weights`` compares the pointer table with the one from before the load --
        only values changed, so ``buffers_generation`` stays and a FramePipeline keeps replaying.  -> torch's result."""
        before, dec = self._weights, self._dec_heads
        res = self.load_state_dict(state_dict, strict=strict)
        if before is None:                       # nothing was packed yet: the first forward does it
            return res
        self._weights = before
        generation = self.buffers_generation
        w = self.refresh_weights()
        if dec is not None and self.buffers_generation == generation:
            # the packed cls / reg branches of the decoder levels: same buffer, new values, written at once (a captured
            # graph with outputs 'camera' / 'all' reads them; decoder_heads() would re-pack only at the next eager call)
            buf, view, _ = dec
            h, lib = self.decoder_heads_struct(), L.lib()
            if lib.tc_decoder_heads_packed_bytes(C.byref(h)) == buf.numel():
                L.check(lib.tc_decoder_heads_pack(C.byref(h), buf.data_ptr(), buf.numel(), C.byref(view),
                                                  L.stream_ptr(buf.device)), 'tc_decoder_heads_pack')
                self._dec_heads = (buf, view, w)
        return res

    def head_weights(self):
        """tc_head_weights over this module's parameters (cached; parameters
        updated in place keep their addresses)."""
        if self._weights is not None:
            return self._weights
        for name, p in self.named_parameters():
            if not (p.is_cuda and p.dtype == torch.float32
                    and p.is_contiguous()):
                raise L.TransCARHipError(
                    'parameter %s must be contiguous fp32 on the GPU (is %s '
                    'on %s); call head.cuda().float()' % (name, p.dtype,
                                                          p.device))
        w = self.weights_struct()
        # one-time re-layout for the fused row-chain kernels (tc_head_pack_weights)
        return self._pack(w, L.lib())

    def _pack(self, w, lib):
        nbytes = L.size_query(lib.tc_head_packed_bytes, C.byref(w))
        dev = self.query_embedding.weight.device
        # Re-pack IN PLACE when the buffer fits (load_state_dict / refresh_weights / a
        # FusionTrainer moving the parameters into its flat bucket): captured hipGraphs hold
        # raw pointers into it.  A new allocation bumps buffers_generation instead.
        if self._packed is None or self._packed.numel() != nbytes or self._packed.device != dev:
            self._packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self.buffers_generation += 1
        self._packed_view = L.tc_head_weights()
        L.check(lib.tc_head_pack_weights(C.byref(w), self._packed.data_ptr(), nbytes, C.byref(self._packed_view),
                                         L.stream_ptr(dev)), 'tc_head_pack_weights')
        self._weights = w
        self._packed_dirty = False
        return w

    def weights_struct(self):
        """tc_head_weights over this module's parameters as they are (no device
        check, nothing packed): what head_weights() hands the library."""
        dec = self.transformer.decoder
        w = L.tc_head_weights()
        w.abi_version = L.TC_ABI_VERSION
        w.num_query, w.embed_dims = self.num_query, self.embed_dims
        w.num_heads = dec.layers[0].attentions[0].num_heads
        if any(ly.attentions[0].num_heads != w.num_heads for ly in dec.layers):
            raise NotImplementedError('MultiheadAttention: num_heads differs between decoder layers')
        L.check_num_heads(w.num_heads)
        # the fusion attention's count rides in the upper half of num_heads (TC_NUM_HEADS_PACK), left 0 at the default 8
        # (radar_num_heads is a public attribute: checked again, and against the modules the unfused training path reads)
        rh = L.check_radar_num_heads(self.radar_num_heads)
        for r in range(L.check_num_fusion_layers(self.num_fusion_layers)):
            if fusion_modules(self, r).attn.num_heads != rh:
                raise L.TransCARHipError('Detr3DHead(HIP): radar_num_heads=%r, but fusion layer %d has an attention of %r heads'
                                         % (rh, r, fusion_modules(self, r).attn.num_heads))
        w.num_heads = L.pack_num_heads(w.num_heads, rh)
        w.ffn_dims = dec.layers[0].ffns[0].feedforward_channels
        if any(ly.ffns[0].feedforward_channels != w.ffn_dims for ly in dec.layers):
            raise NotImplementedError('FFN: feedforward_channels (ffn_dims) differs between decoder layers')
        L.check_ffn_dims(w.ffn_dims)
        w.num_layers = dec.num_layers
        w.num_cams = L.check_num_cams(dec.layers[0].attentions[1].num_cams)
        w.num_levels = dec.layers[0].attentions[1].num_levels
        w.num_points = dec.layers[0].attentions[1].num_points
        for ly in dec.layers:
            ca = ly.attentions[1]
            if (ca.num_cams, ca.num_levels, ca.num_points) != (
                    w.num_cams, w.num_levels, w.num_points):
                raise NotImplementedError(
                    'Detr3DCrossAtten: num_cams / num_levels / num_points '
                    'differ between decoder layers')
        L.check_num_levels(w.num_levels)
        L.check_num_points(w.num_points, w.num_cams, w.num_levels)
        L.check_num_classes(self.cls_out_channels)
        w.num_classes, w.code_size = self.cls_out_channels, self.code_size
        # (public attributes: checked again, and the feature count against the encoder the checkpoint was loaded into)
        w.num_radar_tokens_ref, w.radar_in_dims, _ = L.check_radar_input(self.radar_num_tokens, self.radar_in_dims,
                                                                         self.radar_point_range)
        if self.radar_feat_encoder[0].in_features != w.radar_in_dims:
            raise L.TransCARHipError('Detr3DHead(HIP): radar_in_dims=%r, but radar_feat_encoder.0 takes %d features'
                                     % (w.radar_in_dims, self.radar_feat_encoder[0].in_features))
        for i in range(6):
            w.pc_range[i] = float(self.pc_range[i])
        w.query_embedding = self.query_embedding.weight.data_ptr()
        w.reference_points = _lin(self.transformer.reference_points)
        if not self.with_box_refine and dec.num_layers < 2:
            raise NotImplementedError('with_box_refine=False with a one-layer '
                                      'decoder (its reg branch would refine)')
        for i, ly in enumerate(dec.layers):
            if ly.operation_order != ('self_attn', 'norm', 'cross_attn',
                                      'norm', 'ffn', 'norm'):
                raise NotImplementedError('operation_order %r' %
                                          (ly.operation_order,))
            sa, ca, ffn = ly.attentions[0], ly.attentions[1], ly.ffns[0]
            d = w.layers[i]
            d.self_attn = mha_view(sa.attn)
            d.norm0, d.norm1, d.norm2 = (_ln(n) for n in ly.norms)
            d.attention_weights = _lin(ca.attention_weights)
            d.output_proj = _lin(ca.output_proj)
            d.position_encoder = pos_encoder_view(ca.position_encoder)
            d.ffn0, d.ffn1 = _lin(ffn.layers[0][0]), _lin(ffn.layers[1])
            # without box refinement the decoder gets reg_branches=None
            # (HEAD:271, XFMR:183-203): layers 0 .. L-2 carry NULL branches;
            # the last one is the head's reg_branches[-1] (HEAD:287-293)
            if self.with_box_refine or i == dec.num_layers - 1:
                d.reg = reg_branch_view(self.reg_branches[i])
            else:
                d.reg = L.tc_reg_branch()
        radar_table(self, w, ops._p)
        # (radar_gate is a public attribute: checked again, as num_fusion_layers is)
        for r, pair in enumerate(L.radar_gate_pairs(L.check_radar_gate(self.radar_gate, w.num_radar_layers))):
            w.radar[r].radius_min, w.radar[r].radius_max = pair
        return w

    def decoder_heads_struct(self):
        """tc_decoder_heads over cls_branches / reg_branches as they are (nothing packed)."""
        h = L.tc_decoder_heads()
        h.abi_version = L.TC_ABI_VERSION
        h.num_levels = self.transformer.decoder.num_layers
        h.embed_dims = self.embed_dims
        L.check_num_classes(self.cls_out_channels)
        h.num_classes, h.code_size = self.cls_out_channels, self.code_size
        for i in range(6):
            h.pc_range[i] = float(self.pc_range[i])
        for l in range(h.num_levels):
            h.cls[l] = cls_branch_view(self.cls_branches[l])
            h.reg[l] = reg_branch_view(self.reg_branches[l])
        return h

    def decoder_heads(self):
        """The packed view of cls_branches / reg_branches (tc_decoder_heads_pack), built on first use and again after
        the packed weights were invalidated or a parameter moved."""
        key = self.head_weights()                # (checks the parameters: contiguous fp32 on the GPU; a new object
        #                                           whenever the packed weights were invalidated and built again)
        if self._dec_heads is not None and self._dec_heads[2] is key:
            return self._dec_heads[1]
        h = self.decoder_heads_struct()
        lib = L.lib()
        dev = self.query_embedding.weight.device
        # As `_pack`: written again IN PLACE where the last buffer fits (captured graphs -- FramePipeline lanes and plugin
        # entries with outputs 'camera' / 'all' -- hold raw pointers into it).  A buffer that replaces an older one, or
        # branch parameters at other addresses than the last view named, bump buffers_generation: a stale capture refuses
        # to replay.  (The first buffer bumps nothing: no graph can point at what did not exist.)
        nbytes = L.size_query(lib.tc_decoder_heads_packed_bytes, C.byref(h))
        last = self._dec_heads_last
        buf = last[0] if last is not None else None
        if buf is None or buf.numel() != nbytes or buf.device != dev:
            buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            if last is not None:
                self.buffers_generation += 1
        elif last[1] != bytes(h):
            self.buffers_generation += 1
        self._dec_heads_last = (buf, bytes(h))
        view = L.tc_decoder_heads()
        L.check(lib.tc_decoder_heads_pack(C.byref(h), buf.data_ptr(), buf.numel(), C.byref(view), L.stream_ptr(dev)),
                'tc_decoder_heads_pack')
        self._dec_heads = (buf, view, key)
        return view

    # ------------------------------------------------------------------
    # the f16-range guard's fall-back (`matrix_fallback`) and the options of one launch sequence
    # ------------------------------------------------------------------
    def effective_matrix_path(self, mp):
        """The TC_MATRIX_* path a launch that asks for `mp` runs: f32 iff it asks for f32, or for the automatic path
        after the f16-range guard fell back.  A pinned f16x2 is never touched."""
        return L.TC_MATRIX_F32 if (mp == L.TC_MATRIX_AUTO and self.matrix_fallback) else mp

    def effective_tile_rows(self, rows, mp, derived=False):
        """The tile height next to `effective_matrix_path(mp)`: the 32-row tiles exist on the f16x2 path only, so a 32
        becomes the f32 kernels' 16 where this head turned auto into f32.  An explicit (32, f32) stays, for the library
        to refuse (tc_chain_tile_rows does not lower it) -- unless the rows are `derived` (FusionTrainer's, from its
        look-ahead depth: nobody asked for 32 by name), which an explicit f32 demotes too."""
        if rows == 32 and self.effective_matrix_path(mp) == L.TC_MATRIX_F32 and (derived or mp == L.TC_MATRIX_AUTO):
            return 16
        return rows

    def _options_for(self, options, dev, w, key):
        """The tc_head_options to hand tc_head_forward for the caller's `options`: the f16-range guard's status word
        filled in, the fall-back applied and the camera pre-gather's scratch (one per workspace `key`, sized for the
        weights `w`) where it is asked for without one.  The caller's struct stays as it is; no copy if nothing changes."""
        mp = self.effective_matrix_path(options.matrix_path)
        scratch = options.cam_pregather and not options.cam_pregather_ws
        if options.range_status and mp == options.matrix_path and not scratch:
            return options
        own = L.tc_head_options()
        C.memmove(C.byref(own), C.byref(options), C.sizeof(own))
        if not own.range_status:
            own.range_status = self.status_buffer(dev).data_ptr()
        if mp != own.matrix_path:
            own.chain_tile_rows = self.effective_tile_rows(own.chain_tile_rows, own.matrix_path)
            own.matrix_path = mp
        if scratch:
            pk = ('pregather',) + key
            if pk not in self._workspace:
                self._workspace[pk] = L.device_bytes(dev, L.lib().tc_cam_pregather_workspace_bytes, C.byref(w), key[0])
            own.cam_pregather_ws, own.cam_pregather_bytes = self._workspace[pk].data_ptr(), self._workspace[pk].numel()
        return own

    def _output_views(self, out, levels, B, dev, who):
        """(cls [levels,B,Q,num_classes], box [levels,B,Q,code_size]) over `out`: None = one new allocation; a contiguous
        fp32 buffer of levels * B * Q * (num_classes + code_size) elements (class scores first); or a pair of
        contiguous fp32 tensors of the two shapes' sizes, e.g. slices of a [levels + more,B,Q,.] pair."""
        Q, ncls, code = self.num_query, self.cls_out_channels, self.code_size
        n_cls, n_box = levels * B * Q * ncls, levels * B * Q * code

        def ok(t, n):
            return torch.is_tensor(t) and t.numel() == n and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev
        if isinstance(out, (tuple, list)):
            if len(out) != 2 or not ok(out[0], n_cls) or not ok(out[1], n_box):
                raise L.TransCARHipError('%s: out must be a pair of contiguous fp32 tensors of %d and %d elements on %s'
                                         % (who, n_cls, n_box, dev))
            return out[0].view(levels, B, Q, ncls), out[1].view(levels, B, Q, code)
        if out is None:
            out = torch.empty(n_cls + n_box, dtype=torch.float32, device=dev)
        elif not ok(out, n_cls + n_box):
            raise L.TransCARHipError('%s: out must be a contiguous fp32 buffer of %d elements on %s' % (who, n_cls + n_box, dev))
        out = out.view(-1)
        return out[:n_cls].view(levels, B, Q, ncls), out[n_cls:].view(levels, B, Q, code)

    def all_outputs_buffer(self, B, dev, flat=None):
        """(cls [L + NF,B,Q,num_classes], box [L + NF,B,Q,code_size]) of outputs='all' in one allocation (or over `flat`,
        a contiguous fp32 buffer of that size): decoder levels first; rows [:L] go to decoder_outputs(out=), rows [L:]
        to forward_nhwc(_out=)."""
        return self._output_views(flat, self.transformer.decoder.num_layers + self.num_fusion_layers, B, dev, 'all_outputs_buffer')

    def decoder_level_range(self, levels):
        """(first, count) of decoder_outputs(levels=): None every level, 'last' the last one, or the pair itself."""
        Lyr = self.transformer.decoder.num_layers
        if levels is None or levels == 'all':
            return 0, Lyr
        if levels == 'last':
            return Lyr - 1, 1
        try:
            first, count = (int(v) for v in levels)
        except (TypeError, ValueError):
            raise L.TransCARHipError("decoder_outputs: levels=%r (None, 'last' or (first, count))" % (levels,)) from None
        if first < 0 or count < 1 or first + count > Lyr:
            raise L.TransCARHipError('decoder_outputs: levels=(%d, %d) of a decoder with %d levels' % (first, count, Lyr))
        return first, count

    def decoder_outputs(self, aux_t, options=None, levels=None, out=None):
        """cls_branches[l] / reg_branches[l] of the decoder levels (HEAD:277-298) from the decoder's kept states and
        references (``aux`` of a forward): -> (all_cls_scores [n,B,Q,num_classes], all_bbox_preds [n,B,Q,code_size]).
        levels: None every level (n = L); 'last' or (first, count) that range alone (n = 1 / count) -- the launch is
        n x row tiles, its automatic tile height that of n * B * Q rows.  out: where to write (`_output_views`: a
        caller-owned buffer, e.g. a captured graph's static outputs, or the decoder levels' rows of an 'all' result).
        One launch (tc_decoder_outputs_levels_fwd), enqueue-only."""
        hs = aux_t['inter_states']
        Lyr, B, Q = hs.shape[:3]
        dev = hs.device
        first, count = self.decoder_level_range(levels)
        if Lyr != self.transformer.decoder.num_layers or Q != self.num_query:
            raise L.TransCARHipError('decoder_outputs: inter_states of shape %s, the head has %d levels of %d queries'
                                     % (tuple(hs.shape), self.transformer.decoder.num_layers, self.num_query))
        view = self.decoder_heads()
        cls, box = self._output_views(out, count, B, dev, 'decoder_outputs')
        src = options if options is not None else (self.forward_options if self.forward_options is not None
                                                   else head_options())
        own = L.tc_head_options()          # (of a forward's options this launch takes these three alone)
        own.chain_tile_rows = self.effective_tile_rows(src.chain_tile_rows, src.matrix_path)
        own.matrix_path = self.effective_matrix_path(src.matrix_path)
        own.range_status = src.range_status or self.status_buffer(dev).data_ptr()
        L.check(L.lib().tc_decoder_outputs_levels_fwd(
            C.byref(view), hs.data_ptr(), aux_t['init_reference'].data_ptr(), aux_t['inter_references'].data_ptr(),
            B, Q, first, count, cls.data_ptr(), box.data_ptr(), C.byref(own), L.stream_ptr(dev)),
            'tc_decoder_outputs_levels_fwd')
        return cls, box

    def _check_outputs(self):
        if self.outputs not in OUTPUTS:
            raise ValueError("Detr3DHead: outputs=%r (one of 'fusion', 'camera', 'all')" % (self.outputs,))
        if self.outputs != 'fusion' and self.training:
            raise L.TransCARHipError(
                "Detr3DHead: outputs=%r is not supported in training mode (the decoder is frozen, the decoder levels' "
                "loss terms carry no gradient); use outputs='fusion' or head.eval()" % (self.outputs,))

    def _forward_camera(self, mlvl_feats, img_metas, aux):
        """outputs='camera': the decoder, then its own class / box branches -- no radar anywhere."""
        dev = mlvl_feats[0].device
        feats_nhwc = ops.to_nhwc_levels(mlvl_feats)
        l2i = ops.lidar2img_tensor(img_metas, dev, staged=True)
        img_hw = img_metas[0]['img_shape'][0][:2]
        B = l2i.shape[0]
        # (a decoder-only forward reads no token: the tensor only gives the workspace layout its T)
        tokens = torch.empty((B, 64, self.radar_in_dims), dtype=torch.float32, device=dev)
        base = self.forward_nhwc(feats_nhwc, l2i, img_hw, tokens, 1, aux=True, decoder_only=True,
                                 options=self.forward_options)
        cls, box = self.decoder_outputs(base['aux'])
        outs = {'all_cls_scores': cls, 'all_bbox_preds': box, 'enc_cls_scores': None, 'enc_bbox_preds': None}
        if aux:
            outs['aux'] = base['aux']
        return outs

    def cam_pregather_supported(self):
        """True if this head's shape has the camera pre-gather (_lib.cam_pregather_supported):
        the plugin graphs and a one-lane FramePipeline turn it on only then."""
        ca = self.transformer.decoder.layers[0].attentions[1]
        return L.cam_pregather_supported(self.embed_dims, ca.num_levels, ca.num_cams)

    def check_feature_levels(self, n):
        """The head samples num_levels FPN levels: a forward handed another count raises, naming both."""
        nl = self.transformer.decoder.layers[0].attentions[1].num_levels
        if n != nl:
            raise L.TransCARHipError('Detr3DHead: %d feature levels given, the head has num_levels=%d'
                                     % (n, nl))

    def check_frame_cams(self, lidar2img_cams, B=None, feat_rows=None):
        """The head indexes lidar2img and the feature maps by its num_cams: a frame of another camera count raises
        (_lib.check_frame_cams), naming both, before anything is launched."""
        L.check_frame_cams(self.transformer.decoder.layers[0].attentions[1].num_cams, lidar2img_cams, B, feat_rows)

    def check_frame_nhwc(self, feats_nhwc, lidar2img):
        """check_frame_cams of the device-side entries: lidar2img [B,num_cams,4,4], maps [B*num_cams,H,W,C]"""
        if lidar2img.dim() != 4:
            raise L.TransCARHipError('lidar2img of shape %s, [B,num_cams,4,4] expected' % (tuple(lidar2img.shape),))
        self.check_frame_cams(lidar2img.shape[1], lidar2img.shape[0], [f.shape[0] for f in feats_nhwc])

    def refresh_weights(self):
        """Re-read the parameter pointers and re-pack the weights; call after
        the parameters were changed in place (e.g. an optimizer step) or moved
        (a flat optimizer bucket): captured graphs also hold the un-packed
        pointers (biases, LayerNorm affine), so moved parameters bump
        buffers_generation and a FramePipeline refuses to replay until recapture()."""
        old = bytes(self._weights) if self._weights is not None else None
        self._weights = None
        self._dec_heads = None
        w = self.head_weights()
        if old is not None and bytes(w) != old:
            self.buffers_generation += 1
        return w

    def mark_trainable_dirty(self):
        """The trainable parameters were updated in place (optimizer step on the flat bucket).
        Re-packing them for the fused inference chains is deferred to the next consumer: a
        training iteration never reads the packed radar weights (the frozen decoder's are
        constant, the trainable stack runs on the checkpoint layout), so the 34-launch re-pack
        per iteration was wasted work there."""
        self._packed_dirty = True

    def sync_packed_weights(self):
        """Re-pack the trainable weights now if an optimizer step left them stale (enqueue-only)."""
        if self._packed_dirty and self._weights is not None:
            self.repack_weights(trainable_only=True)
        self._packed_dirty = False

    def repack_weights(self, trainable_only=False):
        """Re-run the weight re-layout into the existing packed buffer: the
        parameters changed IN PLACE (optimizer step on the flat bucket), their
        addresses did not.  Enqueue-only (a few dozen small kernels).
        trainable_only: just the radar / final_* weights (the decoder is frozen
        under tools/train.py:245-252)."""
        if self._weights is None:
            return self.head_weights()
        dev = self.query_embedding.weight.device
        if trainable_only:
            L.check(L.lib().tc_head_repack_trainable(C.byref(self._weights), C.byref(self._packed_view),
                                                     L.stream_ptr(dev)), 'tc_head_repack_trainable')
            return self._weights
        L.check(L.lib().tc_head_pack_weights(C.byref(self._weights), self._packed.data_ptr(), self._packed.numel(),
                                             C.byref(self._packed_view), L.stream_ptr(dev)), 'tc_head_pack_weights')
        return self._weights

    # ------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------
    def radar_tokens(self, img_metas, device, T=None, ingest=None):
        """img_metas[i]['radar'] -> (tokens [B,T,radar_in_dims] on device, pad_mult).

        Raw sweeps (the dict layout of transcar_amd/radar.py, what the devkit returns for HEAD:301-309) are
        turned into the 36-feature rows ON THE DEVICE (``self.radar_ingest == 'device'``, the default:
        tc_radar_build_tokens_batch -- the raw rows go up as they are, one launch builds all samples' tokens;
        float64 arithmetic as HEAD:311-521, bit-equal to the host builder except the six rotated-velocity
        columns, which agree to 1 ulp); [n,36] feature arrays, or ``ingest='host'``, take the numpy route of
        the reference; [n,F] rows given as CUDA tensors are filtered (radar_point_range), compacted and padded on
        the device (tc_radar_pack_rows_batch).  T: fixed token count (default: the smallest multiple of 64 that holds the
        frame, at most radar_num_tokens)."""
        tokens, pad_mult, fill = self._radar_tokens_plan(radar_frames(img_metas), device, T, ingest)
        if fill is not None:
            fill()
        return tokens, pad_mult

    def _radar_tokens_plan(self, raws, device, T=None, ingest=None):
        """-> (tokens [B,T,F], pad_mult, fill).  Device ingest of raw sweeps: `tokens` is allocated but EMPTY and
        ``fill()`` does the work (host packing of the raw rows, three H2D copies per sample, one launch) -- so that
        ``forward`` can enqueue the part of the decoder that does not read the tokens first
        (tc_head_options.phase).  Otherwise the tokens are ready and fill is None: [n,F] rows that are CUDA tensors
        take tc_radar_pack_rows_batch (filter, compaction and padding on the device), numpy rows the host route."""
        mode = ingest or self.radar_ingest
        N, F, rng = L.check_radar_input(self.radar_num_tokens, self.radar_in_dims, self.radar_point_range)
        if F != radar.NUM_FEATURES and any(isinstance(r, dict) for r in raws):
            raise L.TransCARHipError(
                "Detr3DHead(HIP): radar_in_dims=%d: raw radar sweeps give the %d features of the reference; hand "
                "img_metas[i]['radar'] over as [n,%d] feature rows" % (F, radar.NUM_FEATURES, F))
        if mode == 'device' and all(isinstance(r, dict) for r in raws):
            n_raw = [sum(int(np.asarray(r['points'][c]).shape[1]) for c in radar.RADAR_CHANNELS) for r in raws]
            if T is None:
                T = ops.radar_tokens_T(max(n_raw), num_tokens=N)       # n_raw >= the points the range filter keeps
            B = len(raws)
            cap = max(64, ((max(n_raw) + 63) // 64) * 64)
            key = (B, str(device))
            stage = self._radar_stage.get(key)
            if stage is None or stage.cap < cap or stage.num_tokens != N or tuple(stage.point_range) != rng:
                stage = self._radar_stage[key] = ops.RadarRawStage(B, cap, device, point_range=rng, num_tokens=N)
            tokens = torch.empty((B, T, F), dtype=torch.float32, device=device)

            def fill():
                stage.put_all(raws)              # host pack of every sample, then three H2D copies for the batch
                stage.build(tokens)
                if T < N and max(n_raw) > T - 1:
                    ops.radar_check_fits(stage.count, T, N)     # an explicit T: the kept points must fit (one D2H sync)
            return tokens, N - T + 1, fill
        if all(torch.is_tensor(r) and r.is_cuda for r in raws):
            for r in raws:
                if r.dim() != 2 or r.shape[1] != F or r.dtype != torch.float32:
                    raise L.TransCARHipError('radar feature rows must be fp32 [n,%d] tensors (radar_in_dims=%d), got %s %s'
                                             % (F, F, tuple(r.shape), r.dtype))
            n_rows = [int(r.shape[0]) for r in raws]
            if T is None:
                T = ops.radar_tokens_T(max(n_rows), num_tokens=N)
            rows = torch.cat([r.to(device) for r in raws]) if len(raws) > 1 else raws[0].to(device).contiguous()
            offsets = torch.tensor(np.concatenate(([0], np.cumsum(n_rows))), dtype=torch.int32).to(device, non_blocking=True)
            rk = (str(device), rng)
            if self._radar_range is None or self._radar_range[0] != rk:
                self._radar_range = (rk, ops.radar_range_tensor(rng, device))
            tokens, count, pad_mult = ops.radar_pack_rows(rows, offsets, T, N, self._radar_range[1])
            if T < N and max(n_rows) > T - 1:
                ops.radar_check_fits(count, T, N)
            return tokens, pad_mult, None
        raws = [r.detach().cpu().numpy() if torch.is_tensor(r) else r for r in raws]      # (rows as host tensors)
        feats = [radar.build_radar_features(r, point_range=rng, num_features=F) for r in raws]
        if rng != L.RADAR_POINT_RANGE_REF:
            # a range of the head's own applies to prebuilt rows too, as the device route applies it (at the reference's
            # constant the host route takes prebuilt rows as their producer filtered them, as it always has)
            feats = [f[radar.in_range(f, rng)] if not isinstance(r, dict) else f for f, r in zip(feats, raws)]
        tokens, pad_mult = radar.pack_tokens(feats, T=T, num_tokens=N)
        return torch.from_numpy(tokens).to(device), pad_mult, None

    def forward_nhwc(self, feats_nhwc, lidar2img, img_hw, tokens, pad_mult,
                     aux=False, _allow_train=False, lane=0, decoder_only=False,
                     options=None, fill_tokens=None, _out=None):
        """The device-side forward: everything already on the GPU.
        feats_nhwc: list of [B*N,H,W,C]; lidar2img [B,N,4,4]; tokens [B,T,radar_in_dims].
        Only enqueues work on the current stream (graph-capturable).
        lane: forwards that may be in flight at the same time (on different
        streams, transcar_amd/pipeline.py) need different lanes -- each lane
        owns a workspace; the weights are shared.
        decoder_only: stop after the DETR3D decoder (aux carries its states);
        the training iteration recomputes the radar stack itself.
        options: tc_head_options (``head_options(...)``); None = defaults.
        fill_tokens: callable that writes `tokens` (allocated, still empty): the forward is enqueued in two
        phases around it (tc_head_options.phase) -- the decoder layers that do not read the tokens first, so the
        device works while the host packs the radar frame."""
        if not _allow_train:
            require_eval(self)
        self.check_feature_levels(len(feats_nhwc))
        self.check_frame_nhwc(feats_nhwc, lidar2img)
        w = self.head_weights()
        if not decoder_only:
            self.sync_packed_weights()
        packed = self._packed_view
        if decoder_only:
            def _no_radar(src):
                dst = L.tc_head_weights()
                C.memmove(C.byref(dst), C.byref(src), C.sizeof(src))
                dst.num_radar_layers = 0
                return dst
            w, packed = _no_radar(w), _no_radar(packed)
        B = lidar2img.shape[0]
        if tokens.dim() != 3 or tokens.shape[2] != self.radar_in_dims:
            raise L.TransCARHipError('forward_nhwc: tokens of shape %s, the head takes [B,T,%d] (radar_in_dims=%d)'
                                     % (tuple(tokens.shape), self.radar_in_dims, self.radar_in_dims))
        T = tokens.shape[1]
        dev = lidar2img.device
        lib = L.lib()
        key = (B, T, str(dev), int(lane))
        if key not in self._workspace:
            self._workspace[key] = L.device_bytes(dev, lib.tc_head_workspace_bytes, C.byref(w), B, T)
        ws = self._workspace[key]
        options = self._options_for(options if options is not None else head_options(), dev, w, key)
        Q, ncls, code = self.num_query, self.cls_out_channels, self.code_size
        NF = self.num_fusion_layers
        # one allocation, two views (_out: a static buffer of a captured graph, transcar_amd/plugin_graph.py)
        if isinstance(_out, (tuple, list)):
            # a pair (class scores, boxes): the fusion levels' rows of an [L + NF,B,Q,.] result (outputs='all')
            cls, box = self._output_views(_out, NF, B, dev, 'forward_nhwc')
        else:
            out = _out if _out is not None else torch.empty(NF * B * Q * (ncls + code), dtype=torch.float32, device=dev)
            if out.numel() != NF * B * Q * (ncls + code) or out.dtype != torch.float32 or not out.is_contiguous():
                raise L.TransCARHipError('forward_nhwc: _out must be a contiguous fp32 buffer of %d elements' % (NF * B * Q * (ncls + code)))
            cls = out[:NF * B * Q * ncls].view(NF, B, Q, ncls)
            box = out[NF * B * Q * ncls:].view(NF, B, Q, code)
        fv = ops.feats_view(feats_nhwc)
        aux_s, aux_t = None, None
        if aux:
            # aux='train': what a training iteration needs of the frozen decoder (FusionTrainer), its states / references
            # / last box, written in place by the chains -- no init_reference copy, no pair counter (a zero fill + atomics)
            # aux='levels': what decoder_outputs reads (a frame graph with outputs 'camera' / 'all'): the states and the
            # references of every level -- no hit counts, no pair counter
            # a dict: tensors of an earlier call with aux='levels', written again (the two phases of a plugin graph entry
            # are two calls that must share the states)
            Lyr, f32 = w.num_layers, dict(dtype=torch.float32, device=dev)
            if isinstance(aux, dict):
                want = dict(inter_states=(Lyr, B, Q, self.embed_dims), init_reference=(B, Q, 3), inter_references=(Lyr, B, Q, 3))
                for k, shape in want.items():
                    t = aux.get(k)
                    if t is None or tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                        raise L.TransCARHipError('forward_nhwc: aux[%r] must be a contiguous fp32 tensor of shape %s on %s'
                                                 % (k, shape, dev))
                aux_t = {k: aux[k] for k in want}
            else:
                full, levels = aux not in ('train', 'levels'), aux == 'levels'
                aux_t = dict(inter_states=torch.empty((Lyr, B, Q, self.embed_dims), **f32))
                if full or levels:
                    aux_t['init_reference'] = torch.empty((B, Q, 3), **f32)
                aux_t['inter_references'] = torch.empty((Lyr, B, Q, 3), **f32)
                if full:
                    aux_t['radar_hit_counts'] = torch.empty((NF, B, Q), dtype=torch.int32, device=dev)
                if not levels:
                    aux_t['last_box'] = torch.empty((B, Q, code), **f32)
                if full:
                    aux_t['sample_pairs'] = torch.zeros(1, dtype=torch.int64, device=dev)
            aux_s = L.tc_head_aux(**{k: t.data_ptr() for k, t in aux_t.items()})

        def call(opts):
            L.check(lib.tc_head_forward(
                C.byref(w), C.byref(packed), C.byref(fv), B,
                lidar2img.data_ptr(),
                float(img_hw[0]), float(img_hw[1]), tokens.data_ptr(), T,
                int(pad_mult), cls.data_ptr(), box.data_ptr(),
                C.byref(aux_s) if aux_s is not None else None,
                C.byref(opts), ws.data_ptr(), ws.numel(), L.stream_ptr()), 'tc_head_forward')
        if fill_tokens is None:
            call(options)
        elif options.unfused or options.phase != 0:
            fill_tokens()
            call(options)
        else:
            # the copies and the ingest launch go to a side stream: they run beside decoder layers 0 .. L-3
            cur = torch.cuda.current_stream()
            side = self._ingest_streams.get(str(dev))
            if side is None:
                side = self._ingest_streams[str(dev)] = torch.cuda.Stream(device=dev)
            side.wait_stream(cur)                 # (what is already enqueued: an earlier forward may still read
            two = L.tc_head_options()             #  memory the allocator hands out again)
            C.memmove(C.byref(two), C.byref(options), C.sizeof(two))
            two.phase = 1
            call(two)
            with torch.cuda.stream(side):
                fill_tokens()
            tokens.record_stream(side)
            cur.wait_stream(side)
            two.phase = 2
            call(two)
        outs = {'all_cls_scores': cls, 'all_bbox_preds': box,
                'enc_cls_scores': None, 'enc_bbox_preds': None}
        if aux:
            outs['aux'] = aux_t
        return outs

    def forward(self, mlvl_feats, img_metas, aux=False):
        """HEAD:248-261: mlvl_feats list of [B,N,C,H,W]; img_metas list[dict]
        -> dict(all_cls_scores [N,B,Q,10], all_bbox_preds [N,B,Q,10], enc_*), N = num_fusion_layers (3)."""
        self.check_feature_levels(len(mlvl_feats))
        self._check_outputs()
        # (before the plugin graphs look at the call: a frame of another rig never reaches a capture)
        for m in img_metas:
            self.check_frame_cams(len(m['lidar2img']))
        self.check_frame_cams(None, len(img_metas), [f.shape[0] * f.shape[1] if f.dim() == 5 else f.shape[0] for f in mlvl_feats])
        dev = mlvl_feats[0].device
        if dev.type != 'cuda':
            raise L.TransCARHipError(
                'Detr3DHead.forward needs the feature maps on the MI355X '
                '(got %s); transcar_amd has no CPU path' % dev)
        camera = self.outputs == 'camera'
        raws = None if camera else radar_frames(img_metas)   # ('camera' neither reads nor requires radar)
        # round 6: a call signature seen before (same feature-map addresses, shapes, options) replays two captured
        # graphs instead of ~20 eager launches (transcar_amd/plugin_graph.py); anything else takes the eager path below
        if self._plugin_graphs is None:
            from .plugin_graph import PluginGraphs
            self._plugin_graphs = PluginGraphs(self)
        if self._plugin_graphs.eligible(mlvl_feats, img_metas, aux):
            outs = self._plugin_graphs.forward(mlvl_feats, img_metas)
            if outs is not None:
                return outs
        if camera:
            return self._forward_camera(mlvl_feats, img_metas, aux)
        feats_nhwc = ops.to_nhwc_levels(mlvl_feats)       # one launch; channels_last levels zero-copy
        l2i = ops.lidar2img_tensor(img_metas, dev, staged=True)    # pinned ring, one async H2D (none if unchanged)
        img_hw = img_metas[0]['img_shape'][0][:2]           # XFMR:403-404
        tokens, pad_mult, fill = self._radar_tokens_plan(raws, dev)
        if self.training:
            if fill is not None:
                fill()
            return self.forward_train_nhwc(feats_nhwc, l2i, img_hw, tokens,
                                           pad_mult)
        # raw sweeps: the decoder layers that do not read the tokens are enqueued BEFORE the host packs the frame
        if self.outputs == 'all':
            # the default forward with the decoder's states kept, then the decoder levels' own branches; the
            # reference's order with HEAD:607-608 commented out: decoder levels first
            # -- both launches write their rows of ONE [L + NF,B,Q,.] allocation (`all_outputs_buffer`), no torch.cat
            Lyr = self.transformer.decoder.num_layers
            cls, box = self.all_outputs_buffer(len(img_metas), dev)
            outs = self.forward_nhwc(feats_nhwc, l2i, img_hw, tokens, pad_mult, aux=True, fill_tokens=fill,
                                     options=self.forward_options, _out=(cls[Lyr:], box[Lyr:]))
            self.decoder_outputs(outs['aux'], out=(cls[:Lyr], box[:Lyr]))
            outs['all_cls_scores'], outs['all_bbox_preds'] = cls, box
            if not aux:
                del outs['aux']
            return outs
        return self.forward_nhwc(feats_nhwc, l2i, img_hw, tokens, pad_mult,
                                 aux=aux, fill_tokens=fill, options=self.forward_options)

    # ------------------------------------------------------------------
    # training forward: frozen decoder (fused HIP chains, no graph) + the
    # trainable radar stack operator by operator under autograd
    # ------------------------------------------------------------------
    def forward_train_nhwc(self, feats_nhwc, lidar2img, img_hw, tokens,
                           pad_mult):
        """Differentiable forward for one training iteration.

        tools/train.py:245-252 freezes transformer / cls_branches /
        reg_branches / query_embedding, so gradients are only needed in the
        radar encoders, the fusion layers and final_cls*/final_reg*
        (HEAD:531-729).  The frozen decoder runs through tc_head_forward; its
        last state, last reference and last box (``aux``) feed the radar stack,
        which is recomputed here node by node (transcar_amd/autograd_ops.py)
        so that ``loss.backward()`` reaches every trainable parameter through
        HIP backward kernels.  The dropout layers of the fusion layers
        (rf_multihead_attn*.dropout, rf_dropout*, rf_dropout2*, rf_dropout3*;
        p = 0.1 in the reference, HEAD:129-171) are active with counter-based
        masks of (``self.dropout_seed``, rank, number of training forwards so
        far); set their ``p`` to 0 (``set_dropout(0.0)``) for the deterministic
        variant.  The frozen decoder runs in train mode too, as in the
        reference (tools/train.py:245-252 only clears requires_grad): the five
        dropout sites of every decoder layer (``decoder_dropout_p``) draw their
        masks from the same seed."""
        from . import autograd_ops as A
        for grp in (self.transformer, self.cls_branches, self.reg_branches,
                    self.query_embedding):
            for p in grp.parameters():
                if p.requires_grad:
                    raise L.TransCARHipError(
                        'the DETR3D decoder has no backward here: freeze '
                        'transformer / cls_branches / reg_branches / '
                        'query_embedding as tools/train.py:245-252 does '
                        '(Detr3DHead.freeze_decoder())')
        seed = self.next_dropout_seed()
        with torch.no_grad():
            base = self.forward_nhwc(feats_nhwc, lidar2img, img_hw, tokens,
                                     pad_mult, aux=True, _allow_train=True,
                                     options=self.train_options(seed))
        aux = base['aux']
        B, Q, E = aux['inter_states'].shape[1:]
        qf = aux['inter_states'][-1].clone()                  # HEAD:539
        ref_last = aux['inter_references'][-1].contiguous()
        prev_box = aux['last_box']
        cxy, addref = A.radar_reference_l1(ref_last, self.pc_range)

        # radar encoders, HEAD:531-536 (Linear(3,E) runs as K = 4 with a zero column)
        rpe, rfe = self.radar_position_encoder, self.radar_feat_encoder
        T = tokens.shape[1]
        xyz0 = torch.zeros((B, T, 4), dtype=torch.float32, device=tokens.device)
        xyz0[..., :3] = tokens[..., :3]
        w0 = torch.cat((rpe[0].weight, rpe[0].weight.new_zeros(E, 1)), 1)
        u = A.linear(xyz0, w0, rpe[0].bias)
        u = A.add_layernorm(u, None, rpe[1].weight, rpe[1].bias, relu=True)
        u = A.linear(u, rpe[3].weight, rpe[3].bias)
        pos = A.add_layernorm(u, None, rpe[4].weight, rpe[4].bias, relu=True)
        f = A.linear(tokens, rfe[0].weight, rfe[0].bias, act=1)
        f = A.linear(f, rfe[2].weight, rfe[2].bias, act=1)
        f = A.linear(f, rfe[4].weight, rfe[4].bias, act=1)
        mem = pos + f

        all_cls, all_box = [], []
        gate_pairs = L.radar_gate_pairs(L.check_radar_gate(self.radar_gate, self.num_fusion_layers))
        for r in range(self.num_fusion_layers):
            m = fusion_modules(self, r)
            attn = m.attn
            p_attn = float(attn.dropout)
            p_ffn, p2, p3 = float(m.dropout.p), float(m.dropout2.p), float(m.dropout3.p)
            wq, bq = attn.in_proj_weight[:E], attn.in_proj_bias[:E]
            wkv, bkv = attn.in_proj_weight[E:], attn.in_proj_bias[E:]
            qp = A.linear(qf, wq, bq)
            kv = A.linear(mem, wkv, bkv)
            centre, ld_c = (cxy, 2) if r == 0 else (prev_box, self.code_size)
            rmin, rmax = gate_pairs[r]
            ao, hits = A.radar_attn_core(qp, kv, centre, ld_c, prev_box, tokens,
                                         pad_mult, rmin, rmax,
                                         heads=attn.num_heads,
                                         drop=(p_attn, seed, 4 * r + 0, self.radar_num_tokens))
            if p2 > 0.0:            # qf + gate * rf_dropout2(out_proj(ao)), HEAD:581
                y = A.dropout(A.linear(ao, attn.out_proj.weight, attn.out_proj.bias),
                              p2, seed, 4 * r + 1)
                x = qf + y * (hits > 0).unsqueeze(-1).to(y.dtype)
            else:
                x = A.gated_linear_residual(ao, attn.out_proj.weight,
                                            attn.out_proj.bias, qf, hits)
            n2, n3, l1, l2 = m.norm2, m.norm3, m.linear1, m.linear2
            x = A.add_layernorm(x, None, n2.weight, n2.bias)
            h = A.dropout(A.linear(x, l1.weight, l1.bias, act=1), p_ffn, seed, 4 * r + 2)
            ff = A.dropout(A.linear(h, l2.weight, l2.bias), p3, seed, 4 * r + 3)
            qf = A.add_layernorm(x, ff, n3.weight, n3.bias)
            fc, fr = m.final_cls, m.final_reg
            c = A.linear(qf, fc[0].weight, fc[0].bias)
            c = A.add_layernorm(c, None, fc[1].weight, fc[1].bias, relu=True)
            c = A.linear(c, fc[3].weight, fc[3].bias)
            c = A.add_layernorm(c, None, fc[4].weight, fc[4].bias, relu=True)
            c = A.linear(c, fc[6].weight, fc[6].bias)
            t = A.linear(qf, fr[0].weight, fr[0].bias, act=1)
            t = A.linear(t, fr[2].weight, fr[2].bias, act=1)
            t = A.linear(t, fr[4].weight, fr[4].bias)
            box = A.box_add_ref(t, None, addref) if r == 0 else \
                A.box_add_ref(t, prev_box, None)
            all_cls.append(c)
            all_box.append(box)
            prev_box = box
        return {'all_cls_scores': torch.stack(all_cls),
                'all_bbox_preds': torch.stack(all_box),
                'enc_cls_scores': None, 'enc_bbox_preds': None}

    def peek_dropout_seed(self, ahead=1):
        """The seed `next_dropout_seed` will return on its `ahead`-th next call (nothing is advanced): a look-ahead of
        the frozen decoder draws the masks of the iterations that will consume it (FusionTrainer.prefetch_decoder)."""
        return dropout_seed_of(self.dropout_seed, _rank(), self._train_forwards + int(ahead))

    def next_dropout_seed(self):
        """Seed of the counter-based dropout masks of ONE training forward: a function of
        (``self.dropout_seed``, this process's rank, the number of training forwards so far).
        Both training paths (``forward_train_nhwc`` and ``FusionTrainer.step_fused_nhwc``) draw
        from this one counter, so they are seed-compatible; ranks draw different masks as the
        reference's per-process RNG streams do; gradient-accumulation steps (no optimizer step
        in between) get fresh masks."""
        self._train_forwards += 1
        seed = self.last_dropout_seed = dropout_seed_of(self.dropout_seed, _rank(), self._train_forwards)
        return seed

    def set_dropout(self, p, decoder=True):
        """p of every dropout site of the radar fusion layers (HEAD:129-171 build
        them with 0.1) and, with ``decoder``, of the frozen decoder layers
        (CFG:68-80, XFMR:378): 0.0 = the deterministic training forward."""
        for r in range(self.num_fusion_layers):
            m = fusion_modules(self, r)
            m.attn.dropout = float(p)
            for d in (m.dropout, m.dropout1, m.dropout2, m.dropout3):
                d.p = float(p)
        if decoder:
            self.set_decoder_dropout(p)
        return self

    def _decoder_dropout_modules(self):
        for ly in self.transformer.decoder.layers:
            sa, ca, ffn = ly.attentions[0], ly.attentions[1], ly.ffns[0]
            yield sa, ca, ffn

    def set_decoder_dropout(self, p):
        """p of the five dropout sites of every decoder layer."""
        for sa, ca, ffn in self._decoder_dropout_modules():
            sa.attn.dropout = float(p)
            if isinstance(sa.dropout_layer, nn.Dropout):
                sa.dropout_layer.p = float(p)
            elif p > 0:
                sa.dropout_layer = nn.Dropout(float(p))
            ca.dropout.p = float(p)
            ffn.layers[0][2].p = float(p)
            ffn.layers[2].p = float(p)
        return self

    def decoder_dropout_p(self):
        """The dropout probability of the decoder layers in train mode -- one value: the
        HIP path implements the reference configs, where the mmcv wrapper's attention /
        output dropout, the FFN's two dropouts (CFG:68-80) and Detr3DCrossAtten.dropout
        (XFMR:243, 378) are all 0.1."""
        ps = set()
        for sa, ca, ffn in self._decoder_dropout_modules():
            if float(sa.proj_drop.p) != 0.0:
                raise NotImplementedError('MultiheadAttention.proj_drop > 0')
            ps.update((float(sa.attn.dropout), float(getattr(sa.dropout_layer, 'p', 0.0)),
                       float(ca.dropout.p), float(ffn.layers[0][2].p), float(ffn.layers[2].p)))
        if len(ps) != 1:
            raise NotImplementedError('decoder dropout sites with different p: %r' % sorted(ps))
        return ps.pop()

    def train_options(self, seed):
        """tc_head_options of the frozen decoder's forward inside a training iteration."""
        return head_options(decoder_dropout_p=self.decoder_dropout_p() if self.training else 0.0,
                            dropout_seed=seed)

    def freeze_decoder(self):
        """tools/train.py:245-252."""
        for grp in (self.transformer, self.cls_branches, self.reg_branches,
                    self.query_embedding):
            for p in grp.parameters():
                p.requires_grad = False
        return self

    def trainable_parameters(self):
        """(name, parameter) of what one iteration produces a gradient for:
        requires_grad and used by the forward (rf_norm1*, attention_weights2/3,
        output_proj2/3 are constructed but never used, HEAD:191-195)."""
        unused = ('rf_norm1', 'attention_weights2', 'attention_weights3',
                  'output_proj2', 'output_proj3')
        return [(n, p) for n, p in self.named_parameters()
                if p.requires_grad and not n.startswith(unused)]

    def status_buffer(self, device):
        """int32 [1 + 255] on the device: word 0 the f16-range status, the rest scratch for the decode's counts."""
        if self._status_buf is None or self._status_buf.device != torch.device(device):
            self._status_buf = torch.zeros(256, dtype=torch.int32, device=device)
        return self._status_buf

    @property
    def last_range_status(self):
        """0: every forward since the last read stayed inside the f16 planes' range (or ran on the f32 path); 1: a linear
        step of the f16x2 path produced inf / NaN.  Reading it synchronises and clears the word."""
        if self._status_buf is None:
            return 0
        v = int(self._status_buf[0])
        if v:
            self._range_overflow()
        return v

    def _range_overflow(self, pinned=False):
        """The f16-range guard fired (status word 0).  Clears the word; on the automatic matrix path the head falls back
        to the exact-fp32 kernels AND bumps ``buffers_generation`` (round 6): captured graphs -- FramePipeline
        lanes, with the matrix path and the 32-row tiles baked in -- are stale from here on and the pipeline re-captures
        (``matrix_fallback_generation`` names the bump as this one).  With the path pinned to f16x2 nothing can fall back:
        every overflow warns."""
        import warnings
        self._status_buf[:1].zero_()
        if pinned or (self.forward_options is not None and self.forward_options.matrix_path == L.TC_MATRIX_F16X2):
            warnings.warn('transcar_amd: a linear step of the f16x2 matrix path produced a non-finite value and the matrix '
                          'path is pinned to f16x2: the affected rows are inf / NaN in every such forward (matrix_path = '
                          'auto would fall back to the exact-fp32 kernels).')
            return
        if not self.matrix_fallback:
            self.matrix_fallback = True
            self.buffers_generation += 1
            self.matrix_fallback_generation = self.buffers_generation
            warnings.warn('transcar_amd: a linear step of the f16x2 matrix path produced a non-finite value (an activation '
                          'beyond 4.19e6 or a weight beyond 65504 in magnitude, or non-finite inputs); the affected rows '
                          'are inf / NaN.  Forwards with matrix_path = auto run on the exact-fp32 kernels from now on '
                          '(head.matrix_fallback = False to go back).')

    def get_bboxes(self, preds_dicts, img_metas, rescale=False):
        """HEAD:1003-1023."""
        done = None
        if self._plugin_graphs is not None:
            from .plugin_graph import PluginGraphs
            done = PluginGraphs.decoded(preds_dicts)          # the graph of this forward already decoded (same kernel)
        if done is not None:
            preds, status = done
            if status:
                self._range_overflow()
        else:
            sb = self._status_buf if (self._status_buf is not None and
                                      self._status_buf.device == preds_dicts['all_cls_scores'].device) else None
            preds = self.bbox_coder.decode(preds_dicts, z_shift=True, status_buf=sb)
            if getattr(self.bbox_coder, 'last_status', None):
                self._range_overflow()
        ret_list = []
        for i, p in enumerate(preds):
            bboxes = p['bboxes']
            box_type = img_metas[i].get('box_type_3d') if img_metas else None
            if box_type is not None:
                bboxes = box_type(bboxes, 9)
            ret_list.append([bboxes, p['scores'], p['labels']])
        return ret_list

    # ------------------------------------------------------------------
    # training targets and losses (HEAD:742-1001), host/PyTorch as in the reference
    # ------------------------------------------------------------------
    def _get_target_single(self, cls_score, bbox_pred, gt_labels, gt_bboxes):
        """HEAD:742-796."""
        num_bboxes = bbox_pred.size(0)
        res = self.assigner.assign(bbox_pred, cls_score, gt_bboxes, gt_labels)
        pos_inds = torch.nonzero(res.gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        neg_inds = torch.nonzero(res.gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        pos_gt = res.gt_inds[pos_inds] - 1
        labels = gt_bboxes.new_full((num_bboxes,), self.num_classes, dtype=torch.long)
        labels[pos_inds] = gt_labels[pos_gt]
        label_weights = gt_bboxes.new_ones(num_bboxes)
        bbox_targets = torch.zeros_like(bbox_pred)[..., :9]
        bbox_weights = torch.zeros_like(bbox_pred)
        bbox_weights[pos_inds] = 1.0
        bbox_targets[pos_inds] = gt_bboxes[pos_gt]
        return labels, label_weights, bbox_targets, bbox_weights, pos_inds, neg_inds

    def get_targets(self, cls_scores_list, bbox_preds_list, gt_bboxes_list, gt_labels_list):
        """HEAD:798-847."""
        outs = [self._get_target_single(c, b, l, g) for c, b, l, g in
                zip(cls_scores_list, bbox_preds_list, gt_labels_list, gt_bboxes_list)]
        labels, lw, bt, bw, pos, neg = map(list, zip(*outs))
        return (labels, lw, bt, bw, sum(p.numel() for p in pos), sum(n.numel() for n in neg))

    def loss_single(self, cls_scores, bbox_preds, gt_bboxes_list, gt_labels_list):
        """HEAD:849-917 for one radar-layer output [B,Q,*]."""
        num_imgs = cls_scores.size(0)
        labels, lw, bt, bw, num_pos, num_neg = self.get_targets(
            [cls_scores[i] for i in range(num_imgs)], [bbox_preds[i] for i in range(num_imgs)],
            gt_bboxes_list, gt_labels_list)
        labels, lw = torch.cat(labels, 0), torch.cat(lw, 0)
        bbox_targets, bbox_weights = torch.cat(bt, 0), torch.cat(bw, 0)
        cls_scores = cls_scores.reshape(-1, self.cls_out_channels)
        cls_avg_factor = num_pos * 1.0 + num_neg * self.bg_cls_weight
        if self.sync_cls_avg_factor:
            cls_avg_factor = losses.reduce_mean(cls_scores.new_tensor([cls_avg_factor])).item()
        cls_avg_factor = max(cls_avg_factor, 1)
        lc = self.loss_cls_cfg
        loss_cls = losses.sigmoid_focal_loss(
            cls_scores, labels, lw, gamma=lc.get('gamma', 2.0), alpha=lc.get('alpha', 0.25),
            avg_factor=cls_avg_factor, loss_weight=lc.get('loss_weight', 1.0))
        num_pos_t = torch.clamp(losses.reduce_mean(loss_cls.new_tensor([num_pos])), min=1).item()
        bbox_preds = bbox_preds.reshape(-1, bbox_preds.size(-1))
        ntargets = normalize_bbox(bbox_targets, self.pc_range)
        ok = torch.isfinite(ntargets).all(dim=-1)
        bbox_weights = bbox_weights * self.code_weights
        loss_bbox = losses.l1_loss(bbox_preds[ok, :10], ntargets[ok, :10], bbox_weights[ok, :10],
                                   avg_factor=num_pos_t,
                                   loss_weight=self.loss_bbox_cfg.get('loss_weight', 1.0))
        # HEAD:915-916 (the live lines: `loss[torch.isnan(loss)] = 0`; an infinite loss stays infinite)
        return loss_cls.masked_fill(torch.isnan(loss_cls), 0.0), loss_bbox.masked_fill(torch.isnan(loss_bbox), 0.0)

    def loss(self, gt_bboxes_list, gt_labels_list, preds_dicts, gt_bboxes_ignore=None):
        """HEAD:919-1001.  gt boxes: objects with ``gravity_center`` / ``tensor``
        (mmdet3d LiDARInstance3DBoxes) or plain [n,9] gravity-centre tensors.
        PyTorch ops exactly as in the reference (autograd differentiates them);
        ``transcar_amd/device_loss.py`` computes the same values and their
        gradients with three HIP launches and is what ``FusionTrainer`` uses."""
        assert gt_bboxes_ignore is None
        if self.assigner is None:
            raise L.TransCARHipError('loss() needs train_cfg=dict(assigner=...) at construction')
        all_cls, all_box = preds_dicts['all_cls_scores'], preds_dicts['all_bbox_preds']
        device = gt_labels_list[0].device
        gts = []
        for g in gt_bboxes_list:
            if hasattr(g, 'gravity_center'):
                g = torch.cat((g.gravity_center, g.tensor[:, 3:]), dim=1)
            gts.append(g.to(device))
        loss_dict = {}
        per_layer = [self.loss_single(all_cls[i], all_box[i], gts, gt_labels_list)
                     for i in range(len(all_cls))]
        loss_dict['loss_cls'], loss_dict['loss_bbox'] = per_layer[-1]
        for i, (lc, lb) in enumerate(per_layer[:-1]):
            loss_dict['d%d.loss_cls' % i] = lc
            loss_dict['d%d.loss_bbox' % i] = lb
        return loss_dict
