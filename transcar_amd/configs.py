"""Config dicts of the hot path, in the reference's own schema.

``pts_bbox_head`` is the drop-in contract: the three TransCAR configs
(projects/configs/detr3d/detr3d_res101_gridmask.py:51-102 and the _cbgs /
vovnet variants) carry an identical ``pts_bbox_head`` block, so
``build_head(cfg)`` accepts that block unchanged.  Only the FPN level shapes
differ between the ResNet-101 and VoVNet configs.
"""
import copy

point_cloud_range = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
voxel_size = [0.2, 0.2, 8]

pts_bbox_head = dict(
    type='Detr3DHead',
    num_query=900,
    num_classes=10,
    in_channels=256,
    sync_cls_avg_factor=True,
    with_box_refine=True,
    as_two_stage=False,
    transformer=dict(
        type='Detr3DTransformer',
        decoder=dict(
            type='Detr3DTransformerDecoder',
            num_layers=6,
            return_intermediate=True,
            transformerlayers=dict(
                type='DetrTransformerDecoderLayer',
                attn_cfgs=[
                    dict(type='MultiheadAttention', embed_dims=256,
                         num_heads=8, dropout=0.1),
                    dict(type='Detr3DCrossAtten', pc_range=point_cloud_range,
                         num_points=1, embed_dims=256),
                ],
                feedforward_channels=512,
                ffn_dropout=0.1,
                operation_order=('self_attn', 'norm', 'cross_attn', 'norm',
                                 'ffn', 'norm')))),
    bbox_coder=dict(
        type='NMSFreeCoder',
        post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
        pc_range=point_cloud_range,
        max_num=300,
        voxel_size=voxel_size,
        num_classes=10),
    positional_encoding=dict(type='SinePositionalEncoding', num_feats=128,
                             normalize=True, offset=-0.5),
    loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25,
                  loss_weight=2.0),
    loss_bbox=dict(type='L1Loss', loss_weight=0.25),
    loss_iou=dict(type='GIoULoss', loss_weight=0.0))

train_cfg_pts = dict(
    grid_size=[512, 512, 1],
    voxel_size=voxel_size,
    point_cloud_range=point_cloud_range,
    out_size_factor=4,
    assigner=dict(
        type='HungarianAssigner3D',
        cls_cost=dict(type='FocalLossCost', weight=2.0),
        reg_cost=dict(type='BBox3DL1Cost', weight=0.25),
        iou_cost=dict(type='IoUCost', weight=0.0),
        pc_range=point_cloud_range))

#: (H, W) of the four FPN levels the head receives, per backbone config
#: (image padded to 928x1600: transform_3d.py:36; strides from CFG:43-50 and
#: CFG_VOV:39-47).
LEVEL_SHAPES = {
    'res101': [(116, 200), (58, 100), (29, 50), (15, 25)],
    'vovnet': [(232, 400), (116, 200), (58, 100), (29, 50)],
    # tiny maps used by the parity tests (seconds on CPU)
    'tiny': [(8, 12), (4, 6), (2, 3), (1, 2)],
}
IMG_SHAPE = (928, 1600, 3)


def head_cfg(num_query=900, num_points=None, with_box_refine=None,
             num_levels=None, num_heads=None, num_classes=None,
             num_fusion_layers=None, pc_range=None, post_center_range=None, radar_gate=None,
             radar_num_heads=None, radar_num_tokens=None, radar_in_dims=None, radar_point_range=None,
             num_cams=None, feedforward_channels=None):
    """pts_bbox_head; num_points overrides Detr3DCrossAtten.num_points (the
    TransCAR configs use 1, CFG:75; the reference class defaults to 5);
    with_box_refine overrides the head's (the configs: True, CFG:57; the
    reference class defaults to False, HEAD:45); num_levels sets
    Detr3DCrossAtten.num_levels and the transformer's num_feature_levels (the
    configs: the class defaults, 4 FPN levels); num_heads overrides the
    decoder MultiheadAttention's (attn_cfgs[0]; the configs: 8, CFG:69; 4, 8
    or 16 -- the radar fusion attention has its own count, radar_num_heads);
    num_classes sets the head's and the bbox_coder's (the configs: 10, CFG:54
    and :89; 1 .. 32 -- the coder's is the modulus that turns a score index
    into a label, CODER:54-55); num_fusion_layers sets the depth of the radar
    fusion stack (the reference builds 3, HEAD:129-171; 1 .. 3); pc_range sets
    the point-cloud range of the bbox_coder, of every Detr3DCrossAtten and of
    the assigner together (the configs write one ``point_cloud_range`` into all
    three, CFG:74, :85, :112; the result then carries ``train_cfg``, as
    ``train_cfg(pc_range)`` gives it); post_center_range sets the coder's
    (CFG:84).  The radar filter's range does not follow pc_range: the
    reference writes it as a constant (HEAD:304), which is the default of
    radar_point_range.  radar_gate sets the distance gate of
    the fusion layers (``_lib.check_radar_gate``: the reference head's three
    circles with other clamp pairs, or ``dict(type='circle', radii=[R, ...])``,
    the single circle of the paper's radius ablation; the reference writes its
    radii as constants, HEAD:567, 635, 693).  radar_num_heads sets the head
    count of the fusion attention rf_multihead_attn{,2,3} (the reference writes
    8, HEAD:129-171; 4, 8 or 16): the key is added only for a count other than
    8, it adds no parameter.  radar_num_tokens (64 .. 4096), radar_in_dims (4,
    8, .. 64) and radar_point_range set the head's radar input
    (``_lib.check_radar_input``): the tokens attended per frame, the features
    per token (``radar_feat_encoder.0`` becomes Linear(radar_in_dims, 64)) and
    the radar filter's range; the reference writes 1500, 36 and
    +-51.2 / +-51.2 / -5 .. 3 m as constants (HEAD:526, 183, 304), and a key is
    added only for another value.  num_cams sets the cameras per frame of every
    Detr3DCrossAtten and of the transformer (the configs: the class defaults,
    6; 1 .. 16 -- the reference reads the count off ``lidar2img`` and sizes
    ``attention_weights`` as Linear(C, num_cams * num_points * num_levels),
    XFMR:280-292): the keys are added only for a count other than 6.
    feedforward_channels sets the hidden width of every decoder layer's FFN
    (``transformerlayers.feedforward_channels``; the configs: 512, CFG:79; a
    multiple of 256 from 256 to 2048, ``_lib.check_ffn_dims``): the key is
    written only for a width other than 512.  The fusion layers' FFN keeps the
    512 the reference writes as a constant (HEAD:131)."""
    cfg = copy.deepcopy(pts_bbox_head)
    cfg['num_query'] = num_query
    if with_box_refine is not None:
        cfg['with_box_refine'] = bool(with_box_refine)
    if num_points is not None:
        layers = cfg['transformer']['decoder']['transformerlayers']
        layers['attn_cfgs'][1]['num_points'] = int(num_points)
    if num_levels is not None:
        layers = cfg['transformer']['decoder']['transformerlayers']
        layers['attn_cfgs'][1]['num_levels'] = int(num_levels)
        cfg['transformer']['num_feature_levels'] = int(num_levels)
    if num_cams is not None:
        from ._lib import check_num_cams
        if check_num_cams(num_cams) != 6:
            layers = cfg['transformer']['decoder']['transformerlayers']
            layers['attn_cfgs'][1]['num_cams'] = num_cams
            cfg['transformer']['num_cams'] = num_cams
    if feedforward_channels is not None:
        from ._lib import check_ffn_dims
        if check_ffn_dims(feedforward_channels) != 512:
            layers = cfg['transformer']['decoder']['transformerlayers']
            layers['feedforward_channels'] = feedforward_channels
    if num_heads is not None:
        from ._lib import check_num_heads
        check_num_heads(num_heads)
        layers = cfg['transformer']['decoder']['transformerlayers']
        layers['attn_cfgs'][0]['num_heads'] = num_heads
    if num_classes is not None:
        from ._lib import check_num_classes
        check_num_classes(num_classes)
        cfg['num_classes'] = num_classes
        cfg['bbox_coder']['num_classes'] = num_classes
    if num_fusion_layers is not None:
        from ._lib import check_num_fusion_layers
        cfg['num_fusion_layers'] = check_num_fusion_layers(num_fusion_layers)
    if pc_range is not None:
        pc_range = _range6(pc_range, 'pc_range')
        layers = cfg['transformer']['decoder']['transformerlayers']
        layers['attn_cfgs'][1]['pc_range'] = list(pc_range)
        cfg['bbox_coder']['pc_range'] = list(pc_range)
        cfg['train_cfg'] = train_cfg(pc_range)
    if post_center_range is not None:
        cfg['bbox_coder']['post_center_range'] = _range6(post_center_range, 'post_center_range')
    if radar_gate is not None:
        from ._lib import check_radar_gate
        gate = check_radar_gate(radar_gate, cfg.get('num_fusion_layers', 3))
        cfg['radar_gate'] = dict(type=gate['type'], radii=list(gate['radii']))
    if radar_num_heads is not None:
        from ._lib import check_radar_num_heads, TC_RADAR_HEADS
        if check_radar_num_heads(radar_num_heads) != TC_RADAR_HEADS:
            cfg['radar_num_heads'] = radar_num_heads
    if radar_num_tokens is not None or radar_in_dims is not None or radar_point_range is not None:
        from . import _lib as L
        n, f, rng = L.check_radar_input(L.TC_RADAR_TOKENS_REF if radar_num_tokens is None else radar_num_tokens,
                                        L.RADAR_IN_DIMS_REF if radar_in_dims is None else radar_in_dims, radar_point_range)
        if n != L.TC_RADAR_TOKENS_REF:
            cfg['radar_num_tokens'] = n
        if f != L.RADAR_IN_DIMS_REF:
            cfg['radar_in_dims'] = f
        if rng != L.RADAR_POINT_RANGE_REF:
            cfg['radar_point_range'] = list(rng)
    return cfg


def _range6(r, what):
    r = [float(v) for v in r]
    if len(r) != 6 or not all(r[i] < r[i + 3] for i in range(3)):
        raise ValueError('%s=%r: six values (x0, y0, z0, x1, y1, z1), each lower bound below its upper' % (what, r))
    return r


def train_cfg(pc_range=None):
    """train_cfg_pts with ``pc_range`` (None: the configs') as its
    point_cloud_range and the assigner's pc_range."""
    cfg = copy.deepcopy(train_cfg_pts)
    if pc_range is not None:
        cfg['point_cloud_range'] = _range6(pc_range, 'pc_range')
        cfg['assigner']['pc_range'] = _range6(pc_range, 'pc_range')
    return cfg
